"""Patch removal on the device: vitcap_attn_dense_fwd_keys (ops.attn_dense_keys), the dense attention with keys removed per image,
and what is built on it (vitcap_engine_encode_patches / vitcap_engine_prefill_patches through vitcap_amd/model.py).

Bounds.  The op: |err| <= 2e-3 + 2^-7 |want| against the rounding emulation and 4e-3 + 2^-6 |want| against the fp32 softmax over the
visible keys (tests/patch_ref.py), the bounds of tests/test_hip_ops.py::test_attn_dense.  Everything else about the op is bit identity.
Encoder and tag head against the reference under removal masks (tests/golden/reference_patches.npz: the reference's own encoder;
tests/golden/patch_removal.npz: the restated case, recomputed by tests/test_patches_cpu.py): tag logits 2e-2 max abs, activations
1.2e-2 relative L2, the top 50 as a set up to 1e-3 probability ties (tests/test_hip_e2e.py).  Scores and captions: 4e-2 per token,
1e-2 per sequence, tokens equal up to each caption's first decision below GREEDY_MARGIN_FLOOR (tests/test_hip_regions.py).  The entry
points among themselves: bit identity.  Measured figures are printed as MEASURED lines and recorded in docs/LAB_patch_removal.md."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import patch_ref as PR
from conftest import GREEDY_MARGIN_FLOOR, assert_tokens_match_reference

pytestmark = pytest.mark.gpu

SHAPES = [(5, 0), (40, 1), (64, 0), (130, 0), (200, 1), (276, 0), (577, 1), (578, 0)]
NAN16 = 0x7FC0          # bf16 quiet NaN
MAX16 = 0x7F7F          # bf16 largest finite value


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vitcap_amd import ops as o
    return o


@pytest.fixture(scope='module')
def lib(ops):
    from vitcap_amd._lib import lib as l
    return l


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int16)


def _close(got, want, rtol, atol, what):
    n, worst = PR.violations(got, want, rtol, atol)
    assert n == 0, '%s: %d elements off, max err %.3e' % (what, n, worst)
    return worst


@functools.lru_cache(maxsize=None)
def _case(S, bit0):
    """inputs and both CPU references, once per shape"""
    qkv, visible, kinds, garbage = PR.op_case(S, bit0)
    return qkv, visible, kinds, garbage, PR.dense_keys_ref(qkv, visible), PR.dense_keys_ref(qkv, visible, emulate=False)


def _run(ops, qkv, visible, bit0, q_rows=None, garbage=None, extra_words=0):
    B, S = visible.shape
    mask = PR.pack_keys(visible, bit0, garbage, extra_words).cuda().contiguous()
    out = ops.attn_dense_keys(qkv.to(torch.bfloat16).reshape(B * S, 2304).cuda().contiguous(), B, S, mask, bit0=bit0, q_rows=q_rows)
    torch.cuda.synchronize()
    return out.cpu().view(B, S, 768)


# ------------------------------------------------------------------------------------------------ 1: the op
@pytest.mark.parametrize('rows', ['all', 'one'])
@pytest.mark.parametrize('S,bit0', SHAPES)
def test_keys_against_the_emulation(ops, S, bit0, rows):
    """Three images under a mask kind each (patch_ref.OP_KINDS: all kinds over the eight shapes), all query rows and q_rows = 1:
    within test_attn_dense's bounds of the rounding emulation and of the fp32 softmax over the visible keys."""
    qkv, visible, kinds, garbage, want_emu, want_ref = _case(S, bit0)
    n = S if rows == 'all' else 1
    got = _run(ops, qkv, visible, bit0, q_rows=n, garbage=garbage, extra_words=2 if bit0 else 0)
    e1 = _close(got[:, :n], want_emu[:, :n], 2 ** -7, 2e-3, 'keys S=%d bit0=%d %s vs emulation' % (S, bit0, kinds))
    e2 = _close(got[:, :n], want_ref[:, :n], 2 ** -6, 4e-3, 'keys S=%d bit0=%d %s vs fp32 softmax' % (S, bit0, kinds))
    print('MEASURED attn_dense_keys S=%d bit0=%d q_rows=%d %s: max |err| %.3e vs emulation, %.3e vs fp32 softmax' % (S, bit0, n, kinds, e1, e2))
    if rows == 'all' and S >= 40:          # the comparison has teeth: the same output misses the bound of the unmasked attention
        everything = PR.dense_keys_ref(qkv, torch.ones_like(visible))
        assert PR.violations(got, everything)[0] > 100, 'the masks do not matter at S=%d' % S


# ------------------------------------------------------------------------------------------------ 2: all-visible identity
@pytest.mark.parametrize('S,bit0', SHAPES)
def test_every_bit_set_is_the_unmasked_kernel(ops, lib, S, bit0):
    """With every bit set -- rows of exactly the needed words and wider ones -- the bits of vitcap_attn_dense_fwd_rows."""
    qkv = _case(S, bit0)[0]
    B = qkv.shape[0]
    qd = qkv.to(torch.bfloat16).reshape(B * S, 2304).cuda().contiguous()
    ones = torch.ones(B, S, dtype=torch.bool)
    for q_rows in (S, 1):
        want = torch.zeros((B * S, 768), device='cuda', dtype=torch.bfloat16)
        assert lib.vitcap_attn_dense_fwd_rows(_p(qd), _p(want), B, S, q_rows, 0.125, _s()) == 0, lib.vitcap_last_error()
        for extra in (0, 3):
            got = _run(ops, qkv, ones, bit0, q_rows=q_rows, extra_words=extra)
            assert torch.equal(_bits(got[:, :q_rows]), _bits(want.view(B, S, 768)[:, :q_rows])), (q_rows, extra)


# ------------------------------------------------------------------------------------------------ 3: hidden tiles are not read
def _poison(qkv, visible):
    """K and V rows of hidden keys replaced: NaN where the kernel may not read at all (64-key tiles without a visible key, hidden
    left-over keys), bf16-max K and 1e30 V where it reads and must discard (hidden keys of partly visible tiles)."""
    B, S = visible.shape
    nfull, tail, left = PR.key_paths(S)
    q = qkv.to(torch.bfloat16).clone()
    raw = q.view(torch.int16)
    n_nan = n_big = 0
    for b in range(B):
        for t in range((S + PR.KT - 1) // PR.KT):
            lo, hi = t * PR.KT, min(S, (t + 1) * PR.KT)
            hidden = [k for k in range(lo, hi) if not bool(visible[b, k])]
            leftover = t == nfull and left > 0
            for k in hidden:
                if leftover or len(hidden) == hi - lo:
                    raw[b, k, 768:] = NAN16
                    n_nan += 1
                else:
                    raw[b, k, 768:1536] = MAX16
                    q[b, k, 1536:] = 1e30
                    n_big += 1
    return q, n_nan, n_big


@pytest.mark.parametrize('S,bit0', [(130, 0), (200, 1), (276, 0), (577, 1), (578, 0)])
def test_hidden_tiles_and_leftovers_are_not_read(ops, S, bit0):
    """NaN in the K / V rows of wholly hidden tiles and of hidden left-over keys, bf16-max K and 1e30 V in the hidden keys of partly
    hidden tiles: the output bits do not change.  Masks: per image tile 1 hidden (with the left-overs), only tile 1 visible, random
    with the last full tile hidden."""
    qkv = _case(S, bit0)[0]
    g = torch.Generator().manual_seed(77 + S)
    nfull, tail, left = PR.key_paths(S)
    v0 = torch.ones(S, dtype=torch.bool)
    v0[PR.KT:2 * PR.KT] = False
    if left:
        v0[nfull * PR.KT:] = False
    v1 = torch.zeros(S, dtype=torch.bool)
    v1[PR.KT:2 * PR.KT] = True
    v2 = torch.rand(S, generator=g) < 0.5
    v2[(nfull - 1) * PR.KT:nfull * PR.KT] = False
    if left > 1:
        v2[nfull * PR.KT] = False
        v2[nfull * PR.KT + 1] = True
    visible = torch.stack([v0, v1, v2])
    clean = _run(ops, qkv, visible, bit0)
    poisoned, n_nan, n_big = _poison(qkv.view(3, S, 2304), visible)
    assert n_nan >= 3 * PR.KT and n_big >= 16
    B = 3
    mask = PR.pack_keys(visible, bit0).cuda().contiguous()
    got = ops.attn_dense_keys(poisoned.reshape(B * S, 2304).cuda().contiguous(), B, S, mask, bit0=bit0)
    torch.cuda.synchronize()
    got = got.cpu().view(B, S, 768)
    assert not bool(torch.isnan(got.float()).any())
    assert torch.equal(_bits(got), _bits(clean))
    _close(clean, PR.dense_keys_ref(qkv, visible), 2 ** -7, 2e-3, 'S=%d bit0=%d tile masks vs emulation' % (S, bit0))


# ------------------------------------------------------------------------------------------------ 4: an image without a visible key
@pytest.mark.parametrize('S,bit0', [(5, 0), (40, 1), (200, 0), (577, 1)])
def test_image_without_a_visible_key(ops, S, bit0):
    """The middle image hides every key (with garbage in the bits past S): its rows are exact zeros, the neighbours' rows are the
    bits of a launch without it."""
    qkv, visible = _case(S, bit0)[:2]
    visible = visible.clone()
    visible[1] = False
    garbage = torch.tensor([False, True, False])
    got = _run(ops, qkv, visible, bit0, garbage=garbage, extra_words=1)
    assert bool((_bits(got[1]) == 0).all())
    alone = _run(ops, qkv[[0, 2]], visible[[0, 2]], bit0)
    assert torch.equal(_bits(got[[0, 2]]), _bits(alone))


# ------------------------------------------------------------------------------------------------ 5: refusals
def test_keys_refusals(lib):
    B, S = 2, 130
    qd = torch.zeros((B * 160 + 1, 2304), device='cuda', dtype=torch.bfloat16)      # the accepted calls go up to S = 160
    out = torch.zeros((B * 160 + 1, 768), device='cuda', dtype=torch.bfloat16)
    mask = torch.full((B * 6 + 1,), -1, device='cuda', dtype=torch.int32)
    qp, op, mp = qd.data_ptr(), out.data_ptr(), mask.data_ptr()

    def call(q=qp, o=op, B=B, S=S, q_rows=S, m=mp, words=5, bit0=0):
        return lib.vitcap_attn_dense_fwd_keys(C.c_void_p(q), C.c_void_p(o), B, S, q_rows, 0.125, C.c_void_p(m) if m else None, words, bit0, _s())

    assert call() == 0, lib.vitcap_last_error()
    assert call(words=5, bit0=1, S=159) == 0 and call(words=5, S=160) == 0
    for why, kw in (('null mask', dict(m=0)), ('misaligned mask', dict(m=mp + 2)), ('mask_words too small', dict(words=4)),
                    ('mask_words too small under bit0', dict(S=160, bit0=1)), ('bit0 = 2', dict(bit0=2)), ('bit0 = -1', dict(bit0=-1)),
                    ('null qkv', dict(q=0)), ('null out', dict(o=0)), ('B = 0', dict(B=0)), ('S = 0', dict(S=0)), ('q_rows = 0', dict(q_rows=0)),
                    ('q_rows > S', dict(q_rows=S + 1)), ('misaligned qkv', dict(q=qp + 8)), ('misaligned out', dict(o=op + 2)),
                    ('more keys than one wave holds bits for', dict(S=2049, words=65))):
        assert call(**kw) == -1 and b'attn_dense_keys' in lib.vitcap_last_error(), why
    torch.cuda.synchronize()


# ================================================================================================ the engine and the Python surface
HERE = os.path.dirname(os.path.abspath(__file__))
SEQ_TOL, TOK_TOL = 1e-2, 4e-2          # tests/test_hip_regions.py: per sequence / per token against the reference
L8 = PR.CASE_L


@pytest.fixture(scope='module')
def model():
    assert torch.cuda.is_available()
    from vitcap_amd.model import ImageCaptioning
    m = ImageCaptioning(tie_weights=True, tagemb='cls').load_recipe(0).eval()
    m.pack('cuda')
    return m


@pytest.fixture(scope='module')
def case():
    return dict(np.load(os.path.join(HERE, 'golden', PR.CASE_FILE)))


def _images(n, seed=PR.CASE_SEED):
    from vitcap_amd import weights as W
    return torch.from_numpy(W.gen_image_batch(n, seed)).cuda()


def _grid(present578):
    return present578[:, 2:].reshape(-1, 24, 24)


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def _same_top50(got_ids, want_ids, want_prob, what):
    """The top 50 as a set, up to ties: an id of one set missing from the other must sit within 1e-3 of the 50th probability."""
    for b in range(want_ids.shape[0]):
        diff = set(got_ids[b].tolist()) ^ set(want_ids[b].tolist())
        edge = float(want_prob[b].min())
        for t in diff & set(want_ids[b].tolist()):
            p = float(want_prob[b][list(want_ids[b]).index(t)])
            assert p - edge < 1e-3, '%s image %d: tag %d (prob %.4f, 50th %.4f) left the top 50' % (what, b, t, p, edge)
        assert len(diff) <= 4, '%s image %d: %d ids differ' % (what, b, len(diff))


def _check_encoder(model, tags, gold, j, what):
    """tag_patches' results `tags` and the taps against column j of a case file; the bounds of tests/test_hip_e2e.py."""
    B = 2
    logits, topk, prob, tlen = tags
    hid = model.tap('hidden', B, (B, 577, 768)).cpu().numpy()
    tagc = model.tap('tag_hidden', B, (B, 577, 768)).cpu()[:, 0].numpy()
    terr = float(np.abs(logits.cpu().numpy()[:, :64] - gold['tag_logits64'][:, j]).max())
    r_h, r_n = _rel(hid[:, PR.PROBE_ROWS], gold['hidden_probe'][:, j]), _rel(np.linalg.norm(hid, axis=-1), gold['hidden_norms'][:, j])
    r_t = _rel(tagc, gold['tag_cls'][:, j])
    print('MEASURED %s: tag logits[:, :64] max abs %.3e (bound 2e-2); rel L2 hidden probe rows %.3e, hidden row norms %.3e, '
          'tag_hidden[:, 0] %.3e (bound 1.2e-2)' % (what, terr, r_h, r_n, r_t))
    assert terr < 2e-2 and r_h < 1.2e-2 and r_n < 1.2e-2 and r_t < 1.2e-2
    _same_top50(topk.cpu().numpy(), gold['tag_topk'][:, j], gold['tag_prob'][:, j], what)
    assert float(np.abs(prob.cpu().numpy() - np.sort(prob.cpu().numpy(), axis=1)[:, ::-1]).max()) == 0      # best first
    assert np.array_equal(tlen.cpu().numpy(), gold['tag_len'][:, j])


# ------------------------------------------------------------------------------------------------ 6: encoder and tag head
def test_encoder_and_tags_against_the_reference(model, case):
    """tag_patches and the `hidden` / `tag_hidden` taps against the reference's own encoder under two masks that keep patch 575
    (tests/golden/reference_patches.npz) and against the restated case (tests/golden/patch_removal.npz: a 6 x 6 box, the upper half,
    and the all-present control); the decoder's visual rows after the prefill against the case too."""
    img = _images(2)
    ref = dict(np.load(os.path.join(HERE, 'golden', 'reference_patches.npz')))
    for j in range(2):
        _check_encoder(model, model.tag_patches(img, torch.from_numpy(ref['present'][:, j])), ref, j, 'reference mask %d' % j)
    _, pres = PR.case_inputs()
    for j in range(3):
        _check_encoder(model, model.tag_patches(img, _grid(pres[:, j])), case, j, 'case mask %d%s' % (j, ' (all present)' if j == 2 else ''))
        vis = model.tap('vis', 2, (2, 578, 768)).cpu().numpy()
        r_v, r_n = _rel(vis[:, PR.VIS_PROBE_ROWS], case['vis_probe'][:, j]), _rel(np.linalg.norm(vis, axis=-1), case['vis_norms'][:, j])
        print('MEASURED case mask %d: prefill visual rows rel L2 probe rows %.3e, row norms %.3e (bound 1.2e-2)' % (j, r_v, r_n))
        assert r_v < 1.2e-2 and r_n < 1.2e-2
    moved = float((model.tag_patches(img, _grid(pres[:, 0]))[0] - model.tag_patches(img, _grid(pres[:, 2]))[0]).abs().max())
    print('MEASURED the removal moves the device tag logits by %.3f' % moved)
    assert moved > 10 * 2e-2


# ------------------------------------------------------------------------------------------------ 7: scores and captions
def test_scores_and_captions_against_the_reference(model, case):
    """score_patches per token and per sequence, caption_patches token for token up to each caption's first sub-floor margin; at
    least 3 of the 4 removed-patch captions whole."""
    img = _images(2)
    _, pres = PR.case_inputs()
    whole = 0
    for j in range(2):
        grid = _grid(pres[:, j])
        ids, lp = model.caption_patches(img, grid, max_length=L8)
        rep = assert_tokens_match_reference(ids.cpu().numpy(), case['ids'][:, j][:, None], case['margins'][:, j], GREEDY_MARGIN_FLOOR,
                                            min_full=0, what='caption_patches mask %d' % j)
        whole += sum(int(r[2]) for r in rep)
        seq, tok = model.score_patches(img, torch.from_numpy(case['ids'][:, j]), grid, last_tok=torch.from_numpy(case['last'][:, j]),
                                       max_length=L8)
        e_tok = float(np.abs(tok.cpu().numpy() - case['tok_lp'][:, j]).max())
        e_seq = float(np.abs(seq.cpu().numpy() - case['seq_lp'][:, j]).max())
        e_gr = float(np.abs(lp.cpu().numpy()[:, 0] - case['greedy_lp'][:, j]).max())
        print('MEASURED mask %d: score_patches max |d| per token %.3e (bound %.0e), per sequence %.3e (bound %.0e); caption_patches '
              'log-prob %.3e; comparable prefixes %s' % (j, e_tok, TOK_TOL, e_seq, SEQ_TOL, e_gr, [(r[1], r[2]) for r in rep]))
        assert e_tok < TOK_TOL and e_seq < SEQ_TOL
    assert whole >= 3, 'only %d of the 4 captions are comparable as a whole' % whole


# ------------------------------------------------------------------------------------------------ 8: the entry points agree
def test_all_present_is_generate(model):
    img = _images(3, 99)
    ones = torch.ones(3, 24, 24, dtype=torch.bool)
    want_ids, want_lp = model.generate(img, want_tags=True)
    want_logits, want_topk = (x.clone() for x in model.last_tags)
    ids, lp = model.caption_patches(img, ones, want_tags=True)
    assert torch.equal(ids, want_ids) and torch.equal(lp.view(torch.int32), want_lp.view(torch.int32))
    assert torch.equal(model.last_tags[0].view(torch.int32), want_logits.view(torch.int32)) and torch.equal(model.last_tags[1], want_topk)
    logits, topk, prob, tlen = model.tag_patches(img, ones.reshape(3, 576))
    assert torch.equal(logits.view(torch.int32), want_logits.view(torch.int32)) and torch.equal(topk, want_topk)
    assert torch.equal(prob, model.last_tag_probs[0]) and tuple(tlen.shape) == (3,)


def test_crops_are_single_caption_patches_calls(model):
    """caption_crops on the 3 x 3 tiling of 2 images: every (image, tile) result is the bits of a caption_patches / tag_patches call
    on that image alone; caption_with_crops puts the whole-image caption and tags in front."""
    from vitcap_amd.patches import crop_masks
    from vitcap_amd.regions import grid_regions
    img = _images(2)
    boxes = grid_regions(3)
    ids, lp, topk, prob = model.caption_crops(img, boxes, max_length=L8)
    assert tuple(ids.shape) == (2, 9, L8) and tuple(lp.shape) == (2, 9) and tuple(topk.shape) == tuple(prob.shape) == (2, 9, 50)
    present, _ = crop_masks(boxes, 2)
    for b in range(2):
        for r in range(9):
            i1, l1 = model.caption_patches(img[b:b + 1], present[b, r:r + 1], want_tags=True, max_length=L8)
            assert torch.equal(i1[0, 0], ids[b, r]) and torch.equal(l1.view(torch.int32)[0, 0], lp.view(torch.int32)[b, r]), (b, r)
            assert torch.equal(model.last_tags[1][0], topk[b, r]) and torch.equal(model.last_tag_probs[0][0], prob[b, r]), (b, r)
    assert len({tuple(x) for x in ids.view(18, L8).tolist()}) > 1, 'every crop gives the same caption'
    w = model.caption_with_crops(img, boxes, max_length=L8)
    g_ids, g_lp = model.generate(img, want_tags=True, max_length=L8)
    assert torch.equal(w[0], g_ids) and torch.equal(w[1], g_lp) and torch.equal(w[2], model.last_tags[1])
    assert torch.equal(w[4], ids) and torch.equal(w[5], lp) and torch.equal(w[6], topk) and torch.equal(w[7], prob)


# ------------------------------------------------------------------------------------------------ 9: everything else
def test_engine_refusals(model, lib):
    """vitcap_engine_encode_patches / vitcap_engine_prefill_patches refuse a null or misaligned mask, tag_visible > 0 and use_graph,
    naming the cause, and leave the workspace alone."""
    from vitcap_amd import _lib as LB
    img = _images(1)
    model.generate(img)
    ok = model.gen_options(num_beams=1, do_sample=False, num_return_sequences=1, num_keep_best=1, use_graph=False)
    dev = model._packed[2]
    ws, need = model._workspace(1, dev, 0, ok)
    before = model.tap('tag_logits', 1, (1, 30592), opts=ok).clone()
    mask = torch.full((20,), -1, dtype=torch.int32, device=dev)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(o, m, encode):
        mp = C.c_void_p(m) if m else None
        if encode:
            return lib.vitcap_engine_encode_patches(model._engine, C.c_void_p(img.data_ptr()), 0, 1, C.byref(o), C.c_void_p(ws.data_ptr()),
                                                    need, mp, s)
        return lib.vitcap_engine_prefill_patches(model._engine, 1, C.byref(o), C.c_void_p(ws.data_ptr()), need, mp, s)

    for encode in (True, False):
        for o, m, word in ((ok, 0, b'null'), (ok, mask.data_ptr() + 2, b'aligned'),
                           (LB.gen_opts(tag_visible=5, use_graph=0), mask.data_ptr(), b'tag_visible'),
                           (LB.gen_opts(use_graph=1), mask.data_ptr(), b'use_graph')):
            rc = call(o, m, encode)
            assert rc in (-1, -4) and word in lib.vitcap_last_error(), (encode, word, lib.vitcap_last_error())
        assert call(ok, mask.data_ptr(), encode) == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    assert torch.equal(model.tap('tag_logits', 1, (1, 30592), opts=ok).view(torch.int32), before.view(torch.int32))      # all present


def test_encoded_calls_refuse_a_patch_removed_slot(model):
    img = _images(2)
    cap = torch.tensor([[101, 5, 6, 102] + [0] * 16] * 2)
    pres = torch.ones(2, 24, 24, dtype=torch.bool)
    pres[:, :12] = False
    model.caption_patches(img, pres)
    for call in (lambda: model.score_encoded(cap), lambda: model.caption_regions_encoded(torch.tensor([[0, 0, 6, 6]])),
                 lambda: model.attention_maps_encoded(cap), lambda: model.alternatives_encoded(cap),
                 lambda: model.score_masked_encoded(cap, torch.ones(2, 578, dtype=torch.bool)),
                 lambda: model.occlusion_maps_encoded(cap)):
        with pytest.raises(RuntimeError, match='patch-removed'):
            call()
    model.tag_patches(img, pres, slot=3)                   # the state is the slot's
    with pytest.raises(RuntimeError, match='patch-removed'):
        model.score_encoded(cap, slot=3)
    want = model.score(img, cap, one_pass=True)            # an ordinary encoding clears the state
    got = model.score_encoded(cap)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_pipeline_writes_the_crops_tsv(model, tmp_path, monkeypatch):
    """ensure_predict with `crops: 2` on 3 images in batches of 2: one .crops.tsv row per image with 4 records -- rectangle, tags,
    caption and confidence of caption_crops; the prediction TSV is byte-identical to a run without the key."""
    from oracle import vitcap_oracle as O
    from vitcap_amd.patches import to_rows
    from vitcap_amd.pipeline import CaptionUniPipeline
    from vitcap_amd.regions import grid_regions
    monkeypatch.chdir(tmp_path)
    enc = tmp_path / 'enc'
    enc.mkdir()
    toks = ['[PAD]'] + ['w%d' % i for i in range(1, 30522)]
    toks[100], toks[101], toks[102], toks[103] = '[UNK]', '[CLS]', '[SEP]', '[MASK]'
    (enc / 'vocab.txt').write_text('\n'.join(toks) + '\n')
    img = _images(3).cpu()
    keys = ['k%d' % i for i in range(3)]

    def batch(i0, i1):
        n = i1 - i0
        input_ids, am = O.test_text_inputs(n)
        return {'image': img[i0:i1].clone(), 'key': keys[i0:i1], 'input_ids': input_ids, 'attention_mask': am,
                'token_type_ids': torch.zeros(n, 70, dtype=torch.long)}

    def run(name, **kw):
        pl = CaptionUniPipeline(full_expid='E', init_recipe_seed=0, text_encoder_type=str(enc), tagemb='cls', force_predict=True,
                                test_batches=[batch(0, 2), batch(2, 3)], model_file=str(tmp_path / (name + '.pt')), **kw)
        return pl.ensure_predict(), pl

    plain, _ = run('plain')
    with_crops, pl = run('crops', crops=2)
    assert open(plain, 'rb').read() == open(with_crops, 'rb').read()
    crops = with_crops[:-4] + '.crops.tsv'
    assert not os.path.exists(plain[:-4] + '.crops.tsv') and os.path.isfile(crops)
    boxes = grid_regions(2)
    want = []
    for i0, i1 in ((0, 2), (2, 3)):                        # the pipeline's batches
        ids, lp, topk, prob = model.caption_crops(img[i0:i1].cuda(), boxes, gemm_mode=1)
        want += to_rows(ids.cpu(), lp.cpu(), topk.cpu(), prob.cpu(), boxes, pl.tokenizer)
    rows = [l.rstrip('\n').split('\t') for l in open(crops)]
    assert [r[0] for r in rows] == keys
    for b, (key, js) in enumerate(rows):
        recs = json.loads(js)
        assert len(recs) == 4 and recs == want[b]
        assert [rec['rect'] for rec in recs] == [[0, 0, 192, 192], [192, 0, 384, 192], [0, 192, 192, 384], [192, 192, 384, 384]]
        assert all(set(rec) == {'rect', 'caption', 'conf', 'tags'} and 0 < rec['conf'] <= 1 and rec['tags'] for rec in recs)
    for kw, word in ((dict(num_beams=2), 'num_beams'), (dict(use_cbs=True), 'use_cbs'), (dict(tag_visible=3), 'tag_visible'),
                     (dict(regions=2), 'regions'), (dict(occlusion=4), 'occlusion')):
        with pytest.raises(NotImplementedError, match=word):
            run('bad', crops=2, **kw)
    with pytest.raises(ValueError, match='tiling'):
        run('bad', crops=5)
