"""Region captions under beam search on the device: vitcap_attn_decode_beam_groups_masked (ops.attn_decode_beams_masked),
vitcap_engine_generate_beam_masked and vitcap_engine_decode_beam_masked (directly and through vitcap_amd/model.py's
generate_beam(visible=) / caption_regions_beam / caption_with_regions_beam) and the pipeline's `regions_beams: k`.

Bounds.  Attention: beam_masked_ref.bound -- twice what the plain entry point vitcap_attn_decode_beam_groups meets against the same
rounding emulation with everything visible on these inputs (measured by plain_bound() below, recorded in docs/LAB_region_beams.md).
End to end against the reference's beam search on the forward as written with the hidden columns zeroed in the joint mask
(tests/golden/region_beam_captions.npz, recomputed by tests/test_region_beam_cpu.py): scores within 2e-2, the bound of
tests/test_hip_e2e.py::test_image_dependent_beam5_equals_reference; ids through conftest.assert_tokens_match_reference with
BEAM_MARGIN_FLOOR.  Everything else is bit identity.  Region captions have no test against trained weights.  Measured figures are
printed as MEASURED lines."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import beam_masked_ref as BR
from conftest import BEAM_MARGIN_FLOOR, assert_tokens_match_reference

pytestmark = pytest.mark.gpu

SCORE_TOL = 2e-2
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = BR.shapes()


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


def _bits(x):
    return x.contiguous().view(torch.int16)


def _run(ops, vis, cache_dev, step, t, K, gpi, max_len, group_mask=None, words=None, high_bits=False):
    """The masked launch, or with group_mask None the plain entry point vitcap_attn_decode_beam_groups.  -> (B, 2, 768) on the device;
    cache_dev receives the published rows."""
    from vitcap_amd._lib import lib
    n_img, S, B = vis.shape[0], vis.shape[1], step.shape[0]
    q = step.reshape(B * 2, 2304).cuda().contiguous()
    v = vis.reshape(-1, 2304).cuda().contiguous()
    if group_mask is not None:
        mask = BR.pack_bits(group_mask, words=words, high_bits=high_bits).cuda().contiguous()
        out = ops.attn_decode_beams_masked(q, v, cache_dev, mask, n_img, K, S, t, max_len=max_len, groups_per_image=gpi)
    else:
        vt = torch.empty((n_img, 12, 64, 608), device='cuda', dtype=torch.bfloat16)
        out = torch.empty((B * 2, 768), device='cuda', dtype=torch.bfloat16)
        p = lambda x: C.c_void_p(x.data_ptr())
        ops.check(lib.vitcap_attn_beam_vt(p(v), p(vt), n_img, S, None), 'attn_beam_vt')
        ops.check(lib.vitcap_attn_decode_beam_groups(p(q), p(v), p(vt), p(cache_dev), p(out), n_img, K, gpi, S, t, max_len, 0.125, None),
                  'attn_decode_beam_groups')
    torch.cuda.synchronize()
    return out.view(B, 2, 768)


def _within(got, want, what):
    n, worst, a = BR.excess(got, want)
    assert n == 0, '%s: %d elements miss the bound, max |err| %.3e, max |err| - r |want| %.3e' % (what, n, worst, a)
    return a


def plain_bound(ops):
    """What the bound of test 1 is measured with: the PLAIN entry point against the emulation with everything visible, on the random
    and the planted inputs of every shape.  -> the largest |err| - BOUND_R |want| (beam_masked_ref.MEASURED_A must not be below it)."""
    worst = 0.0
    for S, K, t, ml, gpi in SHAPES:
        sets = [BR.random_inputs(S, K, t, ml, gpi)]
        if BR.can_plant(S, K, gpi):
            sets.append(BR.planted_inputs(S, K, t, ml, gpi)[:3])
        for i, (vis, cache, step) in enumerate(sets):
            got = _run(ops, vis, cache.cuda().contiguous(), step, t, K, gpi, ml)
            _, err, a = BR.excess(got, BR.decode_ref(vis, cache, step, t, K, gpi))
            print('MEASURED plain S_vis=%d K=%d t=%d gpi=%d %s: max |err| %.3e, max |err| - r |want| %.3e'
                  % (S, K, t, gpi, ('random', 'planted')[i], err, a))
            worst = max(worst, a)
    print('MEASURED plain entry point, all shapes: a = %.3e' % worst)
    return worst


# ------------------------------------------------------------------------------------------------ 1: the op against the emulation
@pytest.mark.parametrize('S,K,t,ml,gpi', SHAPES)
def test_masked_beam_step_against_the_emulation(ops, S, K, t, ml, gpi):
    """Every group under a mask kind of its own (all kinds of beam_masked_ref.kinds_for(S) over the passes; the bits from S_vis on
    set), random inputs, and the planted inputs under the group masks that hide their dominant keys: per element within the bound.
    The cache rows the step publishes are the step's row 0; no other cache row changes."""
    vis, cache, step = BR.random_inputs(S, K, t, ml, gpi)
    G = BR.N_IMAGES * gpi
    worst = 0.0
    for first in range(0, len(BR.kinds_for(S)), G):
        gm = BR.masks_by_kind(G, S, 60 + S + first, first=first)
        cache_dev = cache.cuda().contiguous()
        got = _run(ops, vis, cache_dev, step, t, K, gpi, ml, gm, high_bits=True)
        worst = max(worst, _within(got, BR.decode_ref(vis, cache, step, t, K, gpi, gm),
                                   'S_vis=%d K=%d t=%d gpi=%d kinds from %d' % (S, K, t, gpi, first)))
        c = cache_dev.cpu()
        assert torch.equal(c[:, t - 1, 0], step[:, 0, 768:1536]) and torch.equal(c[:, t - 1, 1], step[:, 0, 1536:])
        keep = [i for i in range(ml) if i != t - 1]
        assert torch.equal(c[:, keep], cache[:, keep])
    w2 = float('nan')
    if BR.can_plant(S, K, gpi):
        pvis, pcache, pstep, pgm = BR.planted_inputs(S, K, t, ml, gpi)
        got = _run(ops, pvis, pcache.cuda().contiguous(), pstep, t, K, gpi, ml, pgm)
        w2 = _within(got, BR.decode_ref(pvis, pcache, pstep, t, K, gpi, pgm), 'planted S_vis=%d K=%d t=%d gpi=%d' % (S, K, t, gpi))
        n, _, _ = BR.excess(got, BR.decode_ref(pvis, pcache, pstep, t, K, gpi, None))
        assert n > 100, 'the planted keys do not matter'
    print('MEASURED masked S_vis=%d K=%d t=%d gpi=%d: max |err| - r |want| random %.3e, planted %.3e (allowed %.3e)'
          % (S, K, t, gpi, worst, w2, BR.BOUND_MARGIN * BR.MEASURED_A))


# ------------------------------------------------------------------------------------------------ 2: bit identities
@pytest.mark.parametrize('S,K,t,ml,gpi', SHAPES)
def test_all_bits_set_is_the_plain_entry_point(ops, S, K, t, ml, gpi):
    """Every bit set, garbage (all ones) in the bits from S_vis on, in rows of exactly ceil(S_vis / 32) words and in wider ones: `out`
    and the whole cache equal vitcap_attn_decode_beam_groups', bit for bit."""
    vis, cache, step = BR.random_inputs(S, K, t, ml, gpi)
    c0 = cache.cuda().contiguous()
    want = _run(ops, vis, c0, step, t, K, gpi, ml)
    ones = torch.ones(BR.N_IMAGES * gpi, S, dtype=torch.bool)
    for words in (None, (S + 31) // 32 + 3):
        c1 = cache.cuda().contiguous()
        got = _run(ops, vis, c1, step, t, K, gpi, ml, ones, words=words, high_bits=True)
        assert torch.equal(_bits(got), _bits(want)) and torch.equal(c1, c0), 'mask_words=%s' % words


@pytest.mark.parametrize('S,K,t,ml,gpi', [s for s in SHAPES if s[0] >= 578])
def test_skipped_blocks_change_no_bit(ops, S, K, t, ml, gpi):
    """The mask kinds with zero words and zero 16-bit halves -- where the skip path runs -- (a) equal the emulation within the bound
    and (b) with K and V of every hidden key overwritten with +-2^60 (finite) return the bits of the run on the original rows: a
    skipped block adds nothing, a hidden key in a live block weighs exactly 0, no score is read that was not written.  All groups of
    an image carry one kind, so that the keys they hide are hidden from the whole image."""
    vis, cache, step = BR.random_inputs(S, K, t, ml, gpi)
    G = BR.N_IMAGES * gpi
    kinds = ('all_hidden', 'only_0', 'only_last', 'only_16_31', 'hide_32_63', 'hide_128_255', 'only_0_127', 'random')
    gen = torch.Generator().manual_seed(9)
    for i in range(0, len(kinds), BR.N_IMAGES):
        per_img = torch.stack([BR.mask_of_kind(kinds[i + j], S, gen) for j in range(BR.N_IMAGES)])
        gm = per_img.repeat_interleave(gpi, 0)
        assert tuple(gm.shape) == (G, S)
        big = vis.clone()
        sign = torch.where(torch.arange(1536) % 2 == 0, 1.0, -1.0) * 2.0 ** 60
        big[..., 768:] = torch.where(~per_img[..., None], sign.to(torch.bfloat16), vis[..., 768:])
        a = _run(ops, vis, cache.cuda().contiguous(), step, t, K, gpi, ml, gm)
        b = _run(ops, big, cache.cuda().contiguous(), step, t, K, gpi, ml, gm)
        _within(a, BR.decode_ref(vis, cache, step, t, K, gpi, gm), 'kinds %s' % (kinds[i:i + 2],))
        assert bool(torch.isfinite(b.float()).all())
        assert torch.equal(_bits(a), _bits(b)), 'S_vis=%d K=%d t=%d gpi=%d kinds %s' % (S, K, t, gpi, kinds[i:i + 2])


# ------------------------------------------------------------------------------------------------ 3: refusals on the device
def test_attn_decode_beams_masked_refusals(ops):
    """vitcap_attn_decode_beam_groups_masked refuses a null or misaligned mask, too few mask words and what the plain entry point
    refuses, under its own prefix, and leaves the output and the cache alone."""
    from vitcap_amd._lib import lib
    S, K, t, ml, gpi = 47, 2, 1, 20, 1
    vis, cache, step = BR.random_inputs(S, K, t, ml, gpi)
    B = step.shape[0]
    q, v, c = step.reshape(B * 2, 2304).cuda().contiguous(), vis.reshape(-1, 2304).cuda().contiguous(), cache.cuda().contiguous()
    vt = torch.zeros((2, 12, 64, 608), device='cuda', dtype=torch.bfloat16)
    out = torch.full((B * 2, 768), 7.0, dtype=torch.bfloat16, device='cuda')
    mask = torch.full((2, 4), -1, dtype=torch.int32, device='cuda')
    p = lambda x: C.c_void_p(x.data_ptr())

    def f(m, words, K=K, S=S, t=t):
        return lib.vitcap_attn_decode_beam_groups_masked(p(q), p(v), p(vt), p(c), p(out), 2, K, gpi, S, t, ml, 0.125, m, words, None)

    for kw, name in ((dict(m=None, words=2), b'vis_mask is null'), (dict(m=C.c_void_p(mask.data_ptr() + 2), words=2), b'not 4-byte aligned'),
                     (dict(m=p(mask), words=1), b'mask_words'), (dict(m=p(mask), words=2, K=9), b'1..8 sequences'),
                     (dict(m=p(mask), words=2, t=20), b'out of range'), (dict(m=p(mask), words=1, S=16), b'out of range')):
        assert f(**kw) == -1, kw
        assert name in lib.vitcap_last_error() and b'attn_decode_beams_masked' in lib.vitcap_last_error(), (kw, lib.vitcap_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and torch.equal(c.cpu(), cache)
    assert f(p(mask), 4) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


def test_engine_beam_masked_refusals_on_the_device(model):
    """vitcap_engine_generate_beam_masked / vitcap_engine_decode_beam_masked on a bound engine: every refused option returns
    VITCAP_EINVAL with its name and leaves the outputs' sentinel, so does a null mask; the accepted call writes them."""
    from vitcap_amd import _lib as LB
    lib = LB.lib
    img = _images(1, 59).cuda()
    ok = model._beam_masked_options(3, 1.0, 1, {})
    mask = torch.full((8, 19), -1, dtype=torch.int32, device='cuda')
    want = model.generate_beam(img, 3, use_graph=False)                # slot 0 then holds a prefill under the beam options
    fsm = torch.zeros(8, dtype=torch.uint8, device='cuda')
    refused = ((LB.gen_opts(num_beams=1, use_graph=0), b'num_beams'),
               (LB.gen_opts(use_cbs=1, cbs_states=8, num_beams=2, fsm=fsm.data_ptr(), num_constraints=fsm.data_ptr(), use_graph=0), b'use_cbs'),
               (LB.gen_opts(num_beams=3, tag_visible=5, use_graph=0), b'tag_visible'),
               (LB.gen_opts(num_beams=3, use_graph=0, sampling=LB.SampleParams(1, 1.0, 0, 1.0, 0)), b'do_sample'),
               (LB.gen_opts(num_beams=3, use_graph=1), b'use_graph'))
    dev = model._packed[2]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(o, staged, m, forced=None):
        ws, need = model._workspace(1, dev, 0, ok)
        ids = torch.full((1, 1, 20), -7, dtype=torch.int64, device=dev)
        lp = torch.full((1, 1), -7.0, dtype=torch.float32, device=dev)
        mp = C.c_void_p(m.data_ptr()) if m is not None else None
        fp = C.c_void_p(forced.data_ptr()) if forced is not None else None
        if staged:
            rc = lib.vitcap_engine_decode_beam_masked(model._engine, 1, C.byref(o), C.c_void_p(ws.data_ptr()), need, fp, 0,
                                                      C.c_void_p(ids.data_ptr()), C.c_void_p(lp.data_ptr()), None, None, mp, s)
        else:
            rc = lib.vitcap_engine_generate_beam_masked(model._engine, C.c_void_p(img.data_ptr()), 0, 1, C.byref(o),
                                                        C.c_void_p(ws.data_ptr()), need, fp, 0, C.c_void_p(ids.data_ptr()),
                                                        C.c_void_p(lp.data_ptr()), None, None, None, mp, s)
        torch.cuda.synchronize()
        return rc, bool((ids == -7).all()) and bool((lp == -7).all()), ids, lp

    for staged in (True, False):
        for bad, name in refused:
            rc, untouched, _, _ = call(bad, staged, mask)
            assert rc == -1 and name in lib.vitcap_last_error() and b'masked beam decoding' in lib.vitcap_last_error() and untouched, name
        rc, untouched, _, _ = call(ok, staged, mask, forced=torch.full((3, 20), -1, dtype=torch.int64, device=dev))
        assert rc == -1 and b'forced' in lib.vitcap_last_error() and untouched
        rc, untouched, _, _ = call(ok, staged, None)
        assert rc == -1 and b'vis_mask is null' in lib.vitcap_last_error() and untouched
    for staged in (True, False):
        rc, untouched, ids, lp = call(ok, staged, mask)
        assert rc == 0 and not untouched and torch.equal(ids, want[0]) and torch.equal(lp, want[1])


# ------------------------------------------------------------------------------------------------ 4: the engine, everything visible
@pytest.mark.parametrize('K,keep', [(3, 2), (5, 1)])
def test_all_visible_is_generate_beam_without_a_mask(model, K, keep):
    img = _images(2, 56).cuda()
    ids0, lp0 = model.generate_beam(img, K, num_keep_best=keep, use_graph=False)
    ids1, lp1 = model.generate_beam(img, K, num_keep_best=keep, visible=torch.ones(2, 578, dtype=torch.bool), use_graph=False)
    assert tuple(ids1.shape) == (2, keep, 20) and torch.equal(ids0, ids1) and torch.equal(lp0, lp1)
    ids2, lp2 = model.generate_beam(img, K, num_keep_best=keep, visible=torch.ones(2, 24, 24, dtype=torch.bool), use_graph=False)
    assert torch.equal(ids0, ids2) and torch.equal(lp0, lp2)           # the patch grid form keeps the cls columns
    _, lp3 = model.generate_beam(img, K, num_keep_best=keep, visible=torch.zeros(2, 578, dtype=torch.bool), use_graph=False)
    assert not torch.equal(lp0, lp3)                                   # and a mask changes something


# ------------------------------------------------------------------------------------------------ 5: the engine against the reference
@pytest.fixture(scope='module')
def case():
    img, vis = BR.case_inputs()
    return img, vis, dict(np.load(os.path.join(HERE, 'golden', BR.CASE_FILE)))


def test_masked_beam_captions_against_the_reference(model, case):
    """generate_beam(visible=) per mask of the golden case (everything, a 6 x 6 box with the cls tokens, nothing; 3 beams, the 2 best
    kept, max_length 8): scores within 2e-2 of the reference's, ids equal up to each image's first decision whose reference margin is
    below BEAM_MARGIN_FLOOR.  The teeth: the reference's scores under the "nothing" mask lie more than twice the bound from the
    unmasked ones, so a kernel that ignores the mask fails the score check.  The box mask's distance is reported only."""
    img, vis, gold = case
    Lc, K, keep = BR.CASE_L, BR.CASE_K, BR.CASE_KEEP
    sc = gold['scores']
    far = np.abs(sc[:, 2, 0] - sc[:, 0, 0])
    assert (far > 2 * SCORE_TOL).all(), far
    print('MEASURED reference: |nothing - unmasked| %s, |box - unmasked| %s' % (far.tolist(), np.abs(sc[:, 1, 0] - sc[:, 0, 0]).tolist()))
    for j, name in enumerate(BR.CASE_MASKS):
        ids, lp = model.generate_beam(img.cuda(), K, num_keep_best=keep, visible=vis[:, j], max_length=Lc, use_graph=False)
        ids, lp = ids.cpu().numpy(), lp.cpu().numpy()
        d = np.abs(lp - sc[:, j])
        print('MEASURED mask %-8s: max |score - reference| best %.3e, second %.3e; ids equal: %s'
              % (name, d[:, 0].max(), d[:, 1].max(), (ids == gold['ids'][:, j]).all(-1).tolist()))
        assert (d[:, 0] <= SCORE_TOL).all(), (name, lp.tolist(), sc[:, j].tolist())
        # min_full = 0: with random-init weights every caption of this family has a decision below the floor (the golden's margins),
        # so no sequence is comparable as a whole; the prefixes are, and the scores above carry the test
        assert_tokens_match_reference(ids, gold['ids'][:, j], gold['margins'][:, j], BEAM_MARGIN_FLOOR, min_full=0, what='mask ' + name)
    plain = model.generate_beam(img.cuda(), K, num_keep_best=keep, max_length=Lc, use_graph=False)[1].cpu().numpy()
    assert (np.abs(plain[:, 0] - sc[:, 2, 0]) > SCORE_TOL).all()       # the unmasked device result does fail the "nothing" reference


# ------------------------------------------------------------------------------------------------ 6: mask routing
def test_each_image_reads_its_own_mask_row(model):
    """[img0, img0] under [box, nothing] and under [nothing, box]: the results are each other's rows."""
    from vitcap_amd.regions import box_masks
    img = _images(1, 56).cuda().repeat(2, 1, 1, 1).contiguous()
    box, nothing = box_masks(torch.tensor([[9, 9, 15, 15]]))[0], torch.zeros(578, dtype=torch.bool)
    a_ids, a_lp = model.generate_beam(img, 3, num_keep_best=2, visible=torch.stack([box, nothing]), use_graph=False)
    b_ids, b_lp = model.generate_beam(img, 3, num_keep_best=2, visible=torch.stack([nothing, box]), use_graph=False)
    assert torch.equal(a_ids[0], b_ids[1]) and torch.equal(a_ids[1], b_ids[0])
    assert float((a_lp[0] - b_lp[1]).abs().max()) <= 1e-5 and float((a_lp[1] - b_lp[0]).abs().max()) <= 1e-5
    assert float((a_lp[0] - a_lp[1]).abs().max()) > 1e-3               # and the two masks give different results


# ------------------------------------------------------------------------------------------------ 7: the region calls
def test_caption_regions_beam_equals_single_generate_beam_calls(model):
    from vitcap_amd.regions import box_masks, grid_regions
    img = _images(2, 56).cuda()
    boxes = grid_regions(2)
    K, keep = 3, 2
    ids, lp = model.caption_regions_beam(img, boxes, K, num_keep_best=keep)
    assert tuple(ids.shape) == (2, 4, keep, 20) and tuple(lp.shape) == (2, 4, keep) and ids.dtype == torch.int64
    masks = box_masks(boxes)
    for r in range(4):
        ids_r, lp_r = model.generate_beam(img, K, num_keep_best=keep, visible=masks[r:r + 1].expand(2, -1), use_graph=False)
        assert torch.equal(ids[:, r], ids_r) and torch.equal(lp[:, r], lp_r), 'region %d' % r
    ids0, lp0 = model.generate_beam(img, K, num_keep_best=keep)
    ids_w, lp_w, rids, rlp = model.caption_with_regions_beam(img, boxes, K, num_keep_best=keep)
    assert torch.equal(ids_w, ids0) and torch.equal(lp_w, lp0) and torch.equal(rids, ids) and torch.equal(rlp, lp)
    print('MEASURED region beam captions that differ from the whole image\'s: %d of 8' % int((ids[:, :, 0] != ids0[:, None, 0]).any(-1).sum()))


def test_pipeline_writes_the_regions_tsv_by_beam_search(model, tmp_path, monkeypatch):
    """ensure_predict with `regions: 2, regions_beams: 3` on 3 images in batches of 2: the .regions.tsv records are
    caption_regions_beam's best hypotheses; the prediction TSV is byte-identical to a run without the keys."""
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
    with_reg, pl = run('reg', regions=2, regions_beams=3)
    assert open(plain, 'rb').read() == open(with_reg, 'rb').read()
    reg = with_reg[:-4] + '.regions.tsv'
    assert os.path.isfile(reg)
    boxes = grid_regions(2)
    ids = torch.cat([model.caption_regions_beam(img[a:b].cuda(), boxes, 3, gemm_mode=1)[0] for a, b in ((0, 2), (2, 3))])
    lp = torch.cat([model.caption_regions_beam(img[a:b].cuda(), boxes, 3, gemm_mode=1)[1] for a, b in ((0, 2), (2, 3))])
    want = to_rows(ids[:, :, 0].cpu(), lp[:, :, 0].cpu(), boxes, pl.tokenizer)
    rows = [l.rstrip('\n').split('\t') for l in open(reg)]
    assert [r[0] for r in rows] == keys
    for b, (key, js) in enumerate(rows):
        recs = json.loads(js)
        assert len(recs) == 4 and recs == want[b]
        assert all(set(rec) == {'rect', 'caption', 'conf'} and 0 < rec['conf'] <= 1 for rec in recs)
