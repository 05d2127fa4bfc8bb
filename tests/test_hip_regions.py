"""Region captions on the device: vitcap_attn_decode_step_masked (ops.attn_decode_step_masked), vitcap_engine_generate_masked and
vitcap_engine_decode_masked (directly and through vitcap_amd/model.py's generate(visible=) / generate_multi(visible=) /
score_masked(one_pass=False) / caption_regions / caption_regions_encoded) and the pipeline's `regions: g`.

Bounds.  Attention: |err| <= 2e-3 + 2^-7 |want| against the rounding emulation (tests/region_ref.py), the bound of
tests/test_hip_ops.py::test_attn_decode_step.  End to end against the reference's forward as written with the hidden columns zeroed in
the joint mask: 4e-2 per token and 1e-2 per sequence; generated tokens equal the reference's up to each caption's
first decision whose reference margin is below GREEDY_MARGIN_FLOOR (tests/conftest.py).  Everything else is bit
identity.  The reference's side of the end-to-end case is tests/golden/region_captions.npz, which tests/test_region_cpu.py
recomputes.  Measured figures are printed as MEASURED lines and recorded in docs/LAB_regions.md."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import region_ref as RR
from conftest import GREEDY_MARGIN_FLOOR

pytestmark = pytest.mark.gpu

L = RR.LCACHE
EOS, PAD, BOS = 102, 0, 101
SEQ_TOL, TOK_TOL = 1e-2, 4e-2
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vitcap_amd import ops as o
    return o


@pytest.fixture(scope='module')
def model():
    assert torch.cuda.is_available()
    from vitcap_amd.model import ImageCaptioning
    m = ImageCaptioning(tie_weights=True, tagemb='cls').load_recipe(0).eval()
    m.pack('cuda')
    return m


def _images(n, seed=1234):
    from vitcap_amd import weights as W
    return torch.from_numpy(W.gen_image_batch(n, seed))


def _close(got, want, what):
    n, worst = RR.violations(got, want)
    assert n == 0, '%s: %d elements off, max err %.3e' % (what, n, worst)
    return worst


def _run(ops, vis, cache_dev, step, t, spi, visible=None, words=None, high_bits=False):
    """The masked launch, or with visible None the plain one.  -> (B, 2, 768) on the device."""
    B, S = step.shape[0], vis.shape[1]
    q = step.reshape(B * 2, 2304).cuda().contiguous()
    v = vis.reshape(-1, 2304).cuda().contiguous()
    if visible is None:
        out = ops.attn_decode_step(q, v, cache_dev, B, S, t, max_len=L, seq_per_image=spi)
    else:
        mask = RR.pack_bits(visible, words=words, high_bits=high_bits).cuda().contiguous()
        out = ops.attn_decode_step_masked(q, v, cache_dev, mask, B, S, t, max_len=L, seq_per_image=spi)
    torch.cuda.synchronize()
    return out.view(B, 2, 768)


def _bits(x):
    return x.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ 1: the op
SHAPES = [(S, t, spi) for S in (33, 128, 129, 578) for t in (1, 19) for spi in (1, 2)]


@pytest.mark.parametrize('S,t,spi', SHAPES)
def test_masked_step_against_the_emulation(ops, S, t, spi):
    """(a) Every sequence under a mask kind of its own (all kinds of region_ref.kinds_for(S) over the passes), random inputs, and the
    planted inputs under the masks that hide their dominant keys: within the bound of the rounding emulation.  (e) The cache row the
    step publishes is the unmasked kernel's; no other row changes."""
    vis, cache, step = RR.random_inputs(S, spi, t)
    B = step.shape[0]
    worst = 0.0
    for first in range(0, len(RR.kinds_for(S)), B):
        visible = RR.masks_by_kind(B, S, 40 + S + first, first=first)
        cache_dev = cache.cuda().contiguous()
        got = _run(ops, vis, cache_dev, step, t, spi, visible, high_bits=True)        # the bits from S_vis on are ignored
        worst = max(worst, _close(got, RR.decode_ref(vis, cache, step, t, spi, visible),
                                  'masked step S_vis=%d t=%d spi=%d kinds from %d' % (S, t, spi, first)))
        plain = cache.cuda().contiguous()
        _run(ops, vis, plain, step, t, spi)
        assert torch.equal(cache_dev, plain)
        c = cache_dev.cpu()
        assert torch.equal(c[:, t - 1, 0], step[:, 0, 768:1536]) and torch.equal(c[:, t - 1, 1], step[:, 0, 1536:])
        keep = [i for i in range(L) if i != t - 1]
        assert torch.equal(c[:, keep], cache[:, keep])
    pvis, pcache, pstep, pvisible = RR.planted_inputs(S, spi, t)
    got = _run(ops, pvis, pcache.cuda().contiguous(), pstep, t, spi, pvisible)
    w2 = _close(got, RR.decode_ref(pvis, pcache, pstep, t, spi, pvisible), 'planted inputs S_vis=%d t=%d spi=%d' % (S, t, spi))
    n, _ = RR.violations(got, RR.decode_ref(pvis, pcache, pstep, t, spi, None))
    assert n > 100, 'the planted keys do not matter'
    print('MEASURED S_vis=%d t=%d spi=%d: max |err| random %.3e, planted %.3e' % (S, t, spi, worst, w2))


@pytest.mark.parametrize('S,t,spi', SHAPES)
def test_all_bits_set_is_the_unmasked_kernel(ops, S, t, spi):
    """(b) With every bit set -- in rows of exactly ceil(S_vis / 32) words and in wider ones -- the output is vitcap_attn_decode_step's,
    bit for bit."""
    vis, cache, step = RR.random_inputs(S, spi, t)
    B = step.shape[0]
    want = _run(ops, vis, cache.cuda().contiguous(), step, t, spi)
    ones = torch.ones(B, S, dtype=torch.bool)
    for words in (None, (S + 31) // 32 + 3):
        got = _run(ops, vis, cache.cuda().contiguous(), step, t, spi, ones, words=words)
        assert torch.equal(_bits(got), _bits(want)), 'mask_words=%s' % words


@pytest.mark.parametrize('S,t,spi', SHAPES)
def test_hidden_rows_are_not_read_into_the_result(ops, S, t, spi):
    """(c) K and V of every hidden visual key overwritten with +-2^60 (finite): the output equals the run on the original rows bit for
    bit -- a skipped sweep changes nothing, a hidden key weighs exactly 0, and no bit is read at a wrong index.  A key is overwritten
    only where EVERY sequence of its image hides it."""
    vis, cache, step = RR.random_inputs(S, spi, t)
    B = step.shape[0]
    for first in range(0, len(RR.kinds_for(S)), B):
        visible = RR.masks_by_kind(B, S, 40 + S + first, first=first)
        if spi > 1:       # the sequences of an image share its rows: give them one mask kind each pass, so that hidden keys exist
            visible = visible[::spi].repeat_interleave(spi, 0)
        hidden = ~visible.view(B // spi, spi, S).any(1)                # (images, S)
        big = vis.clone()
        sign = torch.where(torch.arange(1536) % 2 == 0, 1.0, -1.0) * 2.0 ** 60
        big[..., 768:] = torch.where(hidden[..., None], sign.to(torch.bfloat16), vis[..., 768:])
        assert bool(torch.isfinite(big.float()).all())
        a = _run(ops, vis, cache.cuda().contiguous(), step, t, spi, visible)
        b = _run(ops, big, cache.cuda().contiguous(), step, t, spi, visible)
        assert bool(torch.isfinite(b.float()).all())
        assert torch.equal(_bits(a), _bits(b)), 'S_vis=%d t=%d spi=%d kinds from %d (%d keys overwritten)' % (S, t, spi, first,
                                                                                                           int(hidden.sum()))


@pytest.mark.parametrize('S,t', [(33, 2), (129, 19), (578, 19)])
def test_masked_step_deterministic_and_sliceable(ops, S, t):
    """(d) Two runs give equal bits, and a batch equals its sequences run one at a time, each with its own mask row."""
    vis, cache, step = RR.random_inputs(S, 1, t)
    B = step.shape[0]
    visible = RR.masks_by_kind(B, S, 77, first=4 if S == 578 else 0)
    a = _run(ops, vis, cache.cuda().contiguous(), step, t, 1, visible)
    b = _run(ops, vis, cache.cuda().contiguous(), step, t, 1, visible)
    assert torch.equal(_bits(a), _bits(b))
    for i in range(B):
        one = _run(ops, vis[i:i + 1], cache[i:i + 1].cuda().contiguous(), step[i:i + 1], t, 1, visible[i:i + 1])
        assert torch.equal(_bits(one), _bits(a[i:i + 1])), 'sequence %d alone differs from the batch' % i


def test_attn_decode_step_masked_refusals(ops):
    """vitcap_attn_decode_step_masked refuses a null or misaligned mask and too few mask words, and leaves the output alone."""
    from vitcap_amd._lib import lib
    vis, cache, step = RR.random_inputs(33, 1, 2)
    B = step.shape[0]
    q, v, c = step.reshape(B * 2, 2304).cuda().contiguous(), vis.reshape(-1, 2304).cuda().contiguous(), cache.cuda().contiguous()
    out = torch.full((B * 2, 768), 7.0, dtype=torch.bfloat16, device='cuda')
    mask = torch.full((B, 4), -1, dtype=torch.int32, device='cuda')
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def f(m, words):
        return lib.vitcap_attn_decode_step_masked(C.c_void_p(q.data_ptr()), C.c_void_p(v.data_ptr()), C.c_void_p(c.data_ptr()),
                                                  C.c_void_p(out.data_ptr()), B, 33, 2, L, 1, 0.125, m, words, s)

    for m, words, name in ((None, 2, b'vis_mask is null'), (C.c_void_p(mask.data_ptr() + 2), 2, b'not 4-byte aligned'),
                           (C.c_void_p(mask.data_ptr()), 1, b'mask_words')):
        assert f(m, words) == -1 and name in lib.vitcap_last_error(), name
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and torch.equal(c.cpu(), cache)
    assert f(C.c_void_p(mask.data_ptr()), 4) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ 2: the engine, everything visible
@pytest.mark.parametrize('streams', [1, 2])
def test_all_visible_is_the_call_without_a_mask(model, streams):
    """generate / generate_multi (fixed seed) / score_masked(one_pass=False) with every key visible return the bits of the calls without
    a mask, on one decode stream and on two."""
    img = _images(2, 56).cuda()
    ones = torch.ones(2, 578, dtype=torch.bool)
    kw = dict(decode_streams=streams, use_graph=False)
    ids0, lp0, tlp0 = model.generate(img, want_token_logprobs=True, **kw)
    ids1, lp1, tlp1 = model.generate(img, want_token_logprobs=True, visible=ones, **kw)
    assert torch.equal(ids0, ids1) and torch.equal(lp0, lp1) and torch.equal(tlp0, tlp1)
    ids2, lp2 = model.generate(img, visible=torch.ones(2, 24, 24, dtype=torch.bool), **kw)      # the patch grid form keeps the cls columns
    assert torch.equal(ids0, ids2) and torch.equal(lp0, lp2)
    m0 = model.generate_multi(img, 3, want_last=True, seed=11, **kw)
    m1 = model.generate_multi(img, 3, want_last=True, seed=11, visible=torch.ones(6, 578, dtype=torch.bool), **kw)
    assert all(torch.equal(a, b) for a, b in zip(m0, m1)) and len(m0) == len(m1) == 3
    caps = ids0[:, 0].cpu().repeat_interleave(2, 0).clone()
    caps[1, 3], caps[3, 5] = 2044, 2045
    caps[3, 7], caps[3, 8:] = EOS, PAD
    s0 = model.score(img, caps, seqs_per_image=2, return_ids=True, **kw)
    s1 = model.score_masked(img, caps, torch.ones(4, 578, dtype=torch.bool), seqs_per_image=2, return_ids=True, one_pass=False, **kw)
    assert all(torch.equal(a, b) for a, b in zip(s0, s1)) and len(s0) == len(s1) == 3
    # and a mask changes something
    _, lp3 = model.generate(img, visible=torch.zeros(2, 578, dtype=torch.bool), **kw)
    assert not torch.equal(lp0, lp3)


# ------------------------------------------------------------------------------------------------ 3: the engine against the reference
@pytest.fixture(scope='module')
def case():
    img, vis = RR.case_inputs()
    return img, vis, dict(np.load(os.path.join(HERE, 'golden', RR.CASE_FILE)))


def test_stepwise_masked_scores_against_the_reference(model, case):
    """(a) The reference's masked greedy captions (two per image, each under its own mask) scored by score_masked(one_pass=False):
    per token within 4e-2 and per sequence within 1e-2 of occlusion_ref.token_logprobs_as_written; (b) the same for
    score_masked(one_pass=True), and the two device paths against each other within the same bounds."""
    img, vis, gold = case
    K, Lc = 2, RR.CASE_L
    caps = torch.from_numpy(gold['ids']).view(2 * K, Lc)
    last = torch.from_numpy(gold['last']).view(2 * K)
    want_tok, want_seq = torch.from_numpy(gold['tok_lp']).view(2 * K, Lc), torch.from_numpy(gold['seq_lp']).view(2 * K)
    visible = vis.view(2 * K, 578)
    got = {}
    for name, one_pass in (('stepwise', False), ('one pass', True)):
        lp, tlp, ids = model.score_masked(img.cuda(), caps, visible, seqs_per_image=K, return_ids=True, last_tok=last, one_pass=one_pass,
                                          max_length=Lc)
        assert torch.equal(ids[:, 0].cpu(), caps)
        got[name] = (lp.cpu(), tlp.cpu())
        d_tok, d_seq = float((got[name][1] - want_tok).abs().max()), float((got[name][0] - want_seq).abs().max())
        print('MEASURED %-8s: max |token_lp - reference| %.3e, max |sequence - reference| %.3e' % (name, d_tok, d_seq))
    d_tok = float((got['stepwise'][1] - got['one pass'][1]).abs().max())
    d_seq = float((got['stepwise'][0] - got['one pass'][0]).abs().max())
    print('MEASURED stepwise against one pass: max token %.3e, max sequence %.3e' % (d_tok, d_seq))
    for name in got:
        assert float((got[name][1] - want_tok).abs().max()) <= TOK_TOL, name
        assert float((got[name][0] - want_seq).abs().max()) <= SEQ_TOL, name
    assert d_tok <= TOK_TOL and d_seq <= SEQ_TOL


def test_generated_region_captions_against_the_reference(model, case):
    """(c) generate(visible=) per mask: ids equal the reference's masked greedy caption token for token up to the first decision whose
    reference margin is below the bf16 noise floor; at most one of the four captions may be cut short by such a margin; the
    log-prob of the whole captions within 1e-2."""
    img, vis, gold = case
    Lc = RR.CASE_L
    whole = 0
    for j in range(2):
        ids, lp = model.generate(img.cuda(), visible=vis[:, j], max_length=Lc)
        ids, lp = ids[:, 0].cpu().numpy(), lp[:, 0].cpu().numpy()
        for b in range(2):
            want, margins = gold['ids'][b, j], gold['margins'][b, j]
            below = np.nonzero(margins[:Lc - 2] < GREEDY_MARGIN_FLOOR)[0]      # the last position is forced to [SEP]
            n_cmp = (int(below[0]) + 1) if len(below) else Lc
            assert (ids[b, :n_cmp] == want[:n_cmp]).all(), 'image %d mask %d: %s against %s' % (b, j, ids[b].tolist(), want.tolist())
            if n_cmp == Lc:
                whole += 1
                assert abs(float(lp[b]) - float(gold['greedy_lp'][b, j])) <= SEQ_TOL
    assert whole >= 3
    differ = sum(int((gold['ids'][b, j] != gold['unmasked_ids'][b]).any()) for b in range(2) for j in range(2))
    assert differ >= 2


# ------------------------------------------------------------------------------------------------ 4: sharing
def test_caption_regions_equals_single_generate_calls(model):
    """R = 9 regions per image (the 3 x 3 tiling: a pass of 8 and a pass of 1 on the first pass's prefill) on 2 images: every caption
    and log-prob equals generate(visible=that region's mask), bit for bit; caption_regions_encoded after a plain generate() gives
    the same; per-image boxes and bool grids are the same regions."""
    from vitcap_amd.regions import box_masks, grid_regions
    img = _images(2, 56).cuda()
    boxes = grid_regions(3)
    ids, lp = model.caption_regions(img, boxes)
    assert tuple(ids.shape) == (2, 9, L) and tuple(lp.shape) == (2, 9) and ids.dtype == torch.int64
    masks = box_masks(boxes)
    for r in range(9):
        ids_r, lp_r = model.generate(img, visible=masks[r:r + 1].expand(2, -1))
        assert torch.equal(ids[:, r], ids_r[:, 0]) and torch.equal(lp[:, r], lp_r[:, 0]), 'region %d' % r
    ids0, lp0 = model.generate(img)                                      # a plain call, one sequence per image, leaves the prefill
    ids_e, lp_e = model.caption_regions_encoded(boxes)
    assert torch.equal(ids_e, ids) and torch.equal(lp_e, lp)
    ids_b, lp_b = model.caption_regions(img, boxes.unsqueeze(0).expand(2, -1, -1))
    grids = masks[:, 2:].view(1, 9, 24, 24).expand(2, -1, -1, -1)
    ids_g, lp_g = model.caption_regions(img, grids)
    assert torch.equal(ids_b, ids) and torch.equal(ids_g, ids) and torch.equal(lp_b, lp) and torch.equal(lp_g, lp)
    ids_w, lp_w, rids, rlp = model.caption_with_regions(img, boxes)
    assert torch.equal(ids_w, ids0) and torch.equal(lp_w, lp0) and torch.equal(rids, ids) and torch.equal(rlp, lp)
    print('MEASURED region captions that differ from the whole image\'s: %d of 18' % int((ids != ids0).any(-1).sum()))


def test_engine_masked_refusals_on_the_device(model):
    """vitcap_engine_generate_masked / vitcap_engine_decode_masked on a bound engine: every refused option returns VITCAP_EINVAL with
    its name and leaves the outputs' sentinel, so does a null mask; the accepted call writes them."""
    from vitcap_amd import _lib as LB
    lib = LB.lib
    img = _images(1, 59).cuda()
    model.generate(img)                                                  # slot 0 holds a prefill for the staged call
    mask = torch.full((8, 19), -1, dtype=torch.int32, device='cuda')
    fsm = torch.zeros(8, dtype=torch.uint8, device='cuda')
    refused = ((LB.gen_opts(num_beams=2, use_graph=0), b'num_beams'),
               (LB.gen_opts(use_cbs=1, cbs_states=8, fsm=fsm.data_ptr(), num_constraints=fsm.data_ptr(), use_graph=0), b'use_cbs'),
               (LB.gen_opts(tag_visible=5, use_graph=0), b'tag_visible'),
               (LB.gen_opts(use_graph=1), b'use_graph'))
    ok = model.gen_options(num_beams=1, do_sample=False, num_return_sequences=1, num_keep_best=1, use_graph=False)
    dev = model._packed[2]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(o, staged, m):
        ws, need = model._workspace(1, dev, 0, ok)
        ids = torch.full((1, 1, 20), -7, dtype=torch.int64, device=dev)
        lp = torch.full((1, 1), -7.0, dtype=torch.float32, device=dev)
        mp = C.c_void_p(m.data_ptr()) if m is not None else None
        if staged:
            rc = lib.vitcap_engine_decode_masked(model._engine, 1, C.byref(o), C.c_void_p(ws.data_ptr()), need, None, 0,
                                                 C.c_void_p(ids.data_ptr()), C.c_void_p(lp.data_ptr()), None, None, mp, s)
        else:
            rc = lib.vitcap_engine_generate_masked(model._engine, C.c_void_p(img.data_ptr()), 0, 1, C.byref(o), C.c_void_p(ws.data_ptr()),
                                                   need, None, 0, C.c_void_p(ids.data_ptr()), C.c_void_p(lp.data_ptr()), None, None, None,
                                                   mp, s)
        torch.cuda.synchronize()
        return rc, bool((ids == -7).all()) and bool((lp == -7).all()), ids, lp

    for staged in (False, True):
        for bad, name in refused:
            rc, untouched, _, _ = call(bad, staged, mask)
            assert rc == -1 and name in lib.vitcap_last_error() and untouched, name
        rc, untouched, _, _ = call(ok, staged, None)
        assert rc == -1 and b'vis_mask is null' in lib.vitcap_last_error() and untouched
    want = model.generate(img, use_graph=False)
    for staged in (False, True):
        rc, untouched, ids, lp = call(ok, staged, mask)
        assert rc == 0 and not untouched and torch.equal(ids, want[0]) and torch.equal(lp, want[1])


# ------------------------------------------------------------------------------------------------ 5: the pipeline
def test_pipeline_writes_the_regions_tsv(model, tmp_path, monkeypatch):
    """ensure_predict with `regions: 2` on 3 images in batches of 2: one .regions.tsv row per image with 4 records whose captions and
    confidences are caption_regions'; the prediction TSV is byte-identical to a run without the key."""
    from oracle import vitcap_oracle as O
    from vitcap_amd.pipeline import CaptionUniPipeline
    from vitcap_amd.regions import grid_regions, to_rows
    monkeypatch.chdir(tmp_path)
    enc = tmp_path / 'enc'
    enc.mkdir()
    toks = ['[PAD]'] + ['w%d' % i for i in range(1, 30522)]
    toks[100], toks[101], toks[102], toks[103] = '[UNK]', '[CLS]', '[SEP]', '[MASK]'
    (enc / 'vocab.txt').write_text('\n'.join(toks) + '\n')
    img = _images(3)
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
    with_reg, pl = run('reg', regions=2)
    assert open(plain, 'rb').read() == open(with_reg, 'rb').read()
    assert not os.path.exists(plain[:-4] + '.regions.tsv')
    reg = with_reg[:-4] + '.regions.tsv'
    assert with_reg.endswith('.predict.tsv') and os.path.isfile(reg)
    boxes = grid_regions(2)
    ids, lp = model.caption_regions(img.cuda(), boxes, gemm_mode=1)      # the predict loop's GEMM mode
    want = to_rows(ids.cpu(), lp.cpu(), boxes, pl.tokenizer)
    rows = [l.rstrip('\n').split('\t') for l in open(reg)]
    assert [r[0] for r in rows] == keys
    for b, (key, js) in enumerate(rows):
        recs = json.loads(js)
        assert len(recs) == 4 and recs == want[b]
        assert [rec['rect'] for rec in recs] == [[0, 0, 192, 192], [192, 0, 384, 192], [0, 192, 192, 384], [192, 192, 384, 384]]
        assert all(set(rec) == {'rect', 'caption', 'conf'} and 0 < rec['conf'] <= 1 and rec['caption'] for rec in recs)
