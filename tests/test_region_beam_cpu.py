"""Region captions under beam search: what is decided without a GPU.

The restatement of the masked beam decode-step attention (tests/beam_masked_ref.py) against region_ref's and against its own
deliberately wrong variants on planted inputs, with the comparator's bound at least ten times below what each of them produces; the
reference's masked beam search against the committed golden (tests/golden/region_beam_captions.npz) and the facts the GPU test
leans on; the refusals of the launcher and of both engine entry points (on an engine without weights, with pointers that are never
followed), of the Python calls (raised before a GPU is touched) and of the pipeline key; the n-best shape of regions.to_rows; and
the refusals the older calls keep."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import beam_masked_ref as BR
import region_ref as RR
from vitcap_amd import regions as RG

BOS, EOS, PAD = 101, 102, 0
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def L():
    from vitcap_amd import _lib
    return _lib


@pytest.fixture(scope='module', autouse=True)
def entry_points(L):
    """Everything here -- the reference included -- is the yardstick of three entry points: without them no test of this file passes."""
    for name in ('vitcap_attn_decode_beam_groups_masked', 'vitcap_engine_decode_beam_masked', 'vitcap_engine_generate_beam_masked'):
        assert name in L.EXPORTS, 'the library does not export ' + name


@pytest.fixture(scope='module')
def model():
    from vitcap_amd.model import ImageCaptioning
    return ImageCaptioning(tie_weights=True, tagemb='cls')


# ------------------------------------------------------------------------------------------------ 1: the restatement
def test_restatement_all_visible_is_region_refs_unmasked_reference():
    for S, K, t, ml, gpi in ((47, 2, 1, 20, 1), (578, 5, 19, 20, 1), (608, 3, 40, 41, 3)):
        vis, cache, step = BR.random_inputs(S, K, t, ml, gpi)
        want = RR.decode_ref(vis, cache, step, t, K * gpi)
        assert torch.equal(BR.decode_ref(vis, cache, step, t, K, gpi), want)
        ones = torch.ones(BR.N_IMAGES * gpi, S, dtype=torch.bool)
        assert torch.equal(BR.decode_ref(vis, cache, step, t, K, gpi, ones), want)
        gm = BR.masks_by_kind(BR.N_IMAGES * gpi, S, 5, first=3)
        assert torch.equal(BR.decode_mutant(vis, cache, step, t, K, gpi, gm, None, emulate=True), BR.decode_ref(vis, cache, step, t, K, gpi, gm))


def test_mask_kinds():
    assert BR.kinds_for(578) == BR.MASK_KINDS == BR.kinds_for(608) and len(BR.MASK_KINDS) == 17
    assert set(BR.kinds_for(47)) == {'random', 'all_hidden', 'only_0', 'only_last', 'bit_31', 'bit_32', 'bit_last', 'bit_15', 'bit_16',
                                     'only_16_31', 'hide_32_63'}
    g = torch.Generator().manual_seed(0)
    m = BR.mask_of_kind('only_16_31', 578, g)
    assert int(m.sum()) == 16 and bool(m[16:32].all())
    m = BR.mask_of_kind('hide_32_63', 47, g)
    assert int((~m).sum()) == 15 and not bool(m[32:].any())
    gm = BR.masks_by_kind(6, 578, 1, first=12)
    assert not bool(gm[0, 16]) and int((~gm[0]).sum()) == 1            # kind 12 + 0 = bit_16
    packed = BR.pack_bits(gm, words=22, high_bits=True)
    assert tuple(packed.shape) == (6, 22) and bool((packed[:, 19:] == -1).all())
    assert BR.shapes()[0] == (47, 2, 1, 20, 1) and len(BR.shapes()) == 24


@pytest.mark.parametrize('S,K,t,ml,gpi', [(578, 5, 19, 20, 1), (578, 2, 1, 20, 3), (578, 3, 40, 41, 1), (608, 8, 19, 20, 1), (47, 2, 1, 20, 1)])
def test_comparator_rejects_each_mutation(S, K, t, ml, gpi):
    """On the planted inputs every mutant misses the bound on more than 100 elements, and by more than ten times the bound."""
    vis, cache, step, gm = BR.planted_inputs(S, K, t, ml, gpi)
    want = BR.decode_ref(vis, cache, step, t, K, gpi, gm, emulate=False)
    if S >= 578:      # the emulation against fp64, under region_ref's bound for that pair (BR.bound is the device against the emulation;
        # with few keys the emulation's own bf16 rounding of P reaches either, tests/test_region_cpu.py)
        n, worst = RR.violations(BR.decode_ref(vis, cache, step, t, K, gpi, gm), want)
        assert n == 0, 'the rounding-emulated restatement misses the bound against fp64: %d elements, max %.3e' % (n, worst)
    for mutate in BR.MUTATIONS:
        got = BR.decode_mutant(vis, cache, step, t, K, gpi, gm, mutate)
        n, worst, _ = BR.excess(got, want)
        ratio = float(((got - want).abs() / BR.bound(want)).max())
        print('MEASURED S_vis=%d K=%d t=%d gpi=%d %-14s: %6d elements off, max |err| %.3f, %.0f times the bound' % (S, K, t, gpi, mutate, n, worst, ratio))
        assert n > 100 and worst > 0.5 and ratio >= 10, (mutate, n, worst, ratio)
    n, worst, _ = BR.excess(BR.decode_ref(vis, cache, step, t, K, gpi, None, emulate=False), want)
    assert n > 100 and worst > 0.5                                     # and the mask matters at all
    assert torch.equal(BR.decode_mutant(vis, cache, step, t, K, gpi, gm, None), want)


def test_bound_is_stated_from_a_measurement():
    """bound(want) = 2 (a + r |want|): r from the number formats, a the measured figure of the plain entry point (LAB section 2)."""
    assert BR.BOUND_R == 2.0 ** -8 and BR.BOUND_MARGIN == 2.0 and 0 < BR.MEASURED_A < 4e-3
    w = torch.tensor([0.0, 1.0, -2.0])
    assert torch.allclose(BR.bound(w), 2 * (BR.MEASURED_A + w.double().abs() / 256))


# ------------------------------------------------------------------------------------------------ 2: the end-to-end reference
def test_the_golden_case_is_the_references(sd_t):
    """Image 0 under its box mask recomputed with the reference's beam driver equals the committed golden; and the facts the GPU test
    leans on: the "nothing" scores lie more than 4e-2 from the unmasked ones, the box ones do not; the box moves image 0's first word."""
    gold = np.load(os.path.join(HERE, 'golden', BR.CASE_FILE))
    assert sorted(gold.files) == ['ids', 'margins', 'scores']
    assert gold['ids'].shape == (2, 3, BR.CASE_KEEP, BR.CASE_L) and gold['margins'].shape == (2, 3, BR.CASE_L - 1)
    case = BR.build_case(sd_t, images=(0,), masks=(1,))
    assert np.array_equal(case['ids'][0, 1], gold['ids'][0, 1])
    assert np.allclose(case['scores'][0, 1], gold['scores'][0, 1], rtol=0, atol=1e-4)
    assert np.allclose(case['margins'][0, 1], gold['margins'][0, 1], rtol=0, atol=1e-4)
    sc = gold['scores'][:, :, 0]
    assert np.allclose(sc, [[-6.4754, -6.4608, -6.5307], [-6.4594, -6.4445, -6.5307]], rtol=0, atol=1e-4)
    assert (np.abs(sc[:, 2] - sc[:, 0]) > 4e-2).all() and (np.abs(sc[:, 1] - sc[:, 0]) < 2e-2).all()
    ids = gold['ids'][:, :, 0]
    assert ids[0, 1, 1] == 18665 and ids[0, 0, 1] == 9138 and (ids[0, 1, 2:] == ids[0, 0, 2:]).all()
    assert [int(p) for p in np.nonzero(ids[0, 2] != ids[0, 0])[0]] == [2, 3, 5] and np.array_equal(ids[0, 2], ids[1, 2])
    assert (gold['scores'][:, :, 0] > gold['scores'][:, :, 1]).all()


def test_masked_stepper_with_everything_visible_is_beam_as_written(sd_t):
    """The masked stepper under the reference's beam driver, all 578 keys visible, gives oracle.beam_as_written's ids and scores (one
    image, 3 beams, the 2 best, max_length 8) -- and they are the golden's unmasked entries."""
    from oracle import vitcap_oracle as O
    img, vis = BR.case_inputs()
    with torch.no_grad():
        ids, lp, _, _ = BR.beam_masked(sd_t, img[:1], vis[:1, 0], BR.CASE_K, BR.CASE_L, num_keep_best=BR.CASE_KEEP)
        want_ids, want_lp = O.beam_as_written(sd_t, img[:1], BR.CASE_K, max_length=BR.CASE_L, num_keep_best=BR.CASE_KEEP)
    assert torch.equal(ids, want_ids) and float((lp - want_lp).abs().max()) < 1e-5
    gold = np.load(os.path.join(HERE, 'golden', BR.CASE_FILE))
    assert np.array_equal(ids[0].numpy(), gold['ids'][0, 0]) and np.allclose(lp[0].numpy(), gold['scores'][0, 0], rtol=0, atol=1e-4)


# ------------------------------------------------------------------------------------------------ 3: the C entry points
def test_attn_decode_beams_masked_launcher_refuses_bad_arguments(L):
    """Every refusal of vitcap_attn_decode_beam_groups_masked comes before anything is enqueued, so it can be met without a device."""
    lib = L.lib
    buf = (C.c_char * 1024)()
    a = C.c_void_p((C.addressof(buf) + 255) & ~255)

    def f(q=a, vis=a, vt=a, cache=a, out=a, n=1, K=3, gpi=1, S=578, t=1, ml=20, mask=a, words=19):
        return lib.vitcap_attn_decode_beam_groups_masked(q, vis, vt, cache, out, n, K, gpi, S, t, ml, 0.125, mask, words, None)

    for kw, name in (({'mask': None}, b'vis_mask is null'), ({'mask': C.c_void_p(a.value + 1)}, b'vis_mask is not 4-byte aligned'),
                     ({'mask': C.c_void_p(a.value + 2)}, b'vis_mask is not 4-byte aligned'), ({'words': 18}, b'mask_words'),
                     ({'S': 47, 'words': 1}, b'mask_words'), ({'words': 0}, b'mask_words'), ({'S': 0}, b'mask_words'),
                     ({'t': 0}, b'out of range'), ({'t': 20}, b'out of range'), ({'ml': 42, 't': 41}, b'out of range'),
                     ({'S': 609, 'words': 20}, b'out of range'), ({'S': 16}, b'out of range'), ({'K': 0}, b'1..8 sequences'),
                     ({'K': 9}, b'1..8 sequences'), ({'q': None}, b'bad arguments'), ({'vt': None}, b'bad arguments'),
                     ({'out': None}, b'bad arguments'), ({'n': 0}, b'bad arguments'), ({'gpi': 0}, b'bad arguments')):
        assert f(**kw) == -1, kw
        assert b'attn_decode_beams_masked:' in lib.vitcap_last_error() and name in lib.vitcap_last_error(), (kw, lib.vitcap_last_error())
    # the plain entry points keep their prefix
    assert lib.vitcap_attn_decode_beam_groups(a, a, a, a, a, 1, 9, 1, 578, 1, 20, 0.125, None) == -1
    assert lib.vitcap_last_error().startswith(b'attn_decode_beams: 1..8 sequences')


def test_engine_beam_masked_entry_points_refuse_without_a_device(L):
    """vitcap_engine_decode_beam_masked / vitcap_engine_generate_beam_masked on an engine without weights: every refused option
    returns VITCAP_EINVAL with its name before anything else is looked at; an accepted call gets as far as the unbound engine."""
    lib = L.lib
    h = C.c_void_p()
    assert lib.vitcap_engine_create(C.byref(h)) == 0 and h.value
    buf = (C.c_char * 1024)()
    a = C.c_void_p((C.addressof(buf) + 255) & ~255)

    def decode(o, mask=a, B=1, forced=None, tok=None):
        return lib.vitcap_engine_decode_beam_masked(h, B, C.byref(o) if o is not None else None, a, 1 << 40, forced, 0, a, a, tok, None, mask,
                                                    None)

    def generate(o, mask=a, B=1, forced=None, tok=None):
        return lib.vitcap_engine_generate_beam_masked(h, a, 0, B, C.byref(o) if o is not None else None, a, 1 << 40, forced, 0, a, a, tok, None,
                                                      None, mask, None)

    refused = ((L.gen_opts(num_beams=1, use_graph=0), b'num_beams'), (None, b'num_beams'),
               (L.gen_opts(num_beams=2, use_cbs=1, cbs_states=8, fsm=4096, num_constraints=4096, use_graph=0), b'use_cbs'),
               (L.gen_opts(num_beams=3, tag_visible=5, use_graph=0), b'tag_visible'),
               (L.gen_opts(num_beams=3, use_graph=0, sampling=L.SampleParams(1, 1.0, 0, 1.0, 0)), b'do_sample'),
               (L.gen_opts(num_beams=3, use_graph=1), b'use_graph'))
    for fn in (decode, generate):
        for o, name in refused:
            assert fn(o) == -1 and name in lib.vitcap_last_error() and b'masked beam decoding' in lib.vitcap_last_error(), name
        for k in (2, 5, 8):
            ok = L.gen_opts(num_beams=k, num_keep_best=2, length_penalty=0.7, repetition_penalty=1.2, use_graph=0)
            assert fn(ok, forced=a) == -1 and b'forced' in lib.vitcap_last_error()
            assert fn(ok, tok=a) == -1 and b'forced' in lib.vitcap_last_error()
            assert fn(ok, mask=None) == -1 and b'vis_mask is null' in lib.vitcap_last_error()
            assert fn(ok, mask=C.c_void_p(a.value + 2)) == -1 and b'vis_mask is not 4-byte aligned' in lib.vitcap_last_error()
            assert fn(ok, B=0) == -1 and b'bad batch' in lib.vitcap_last_error()
            assert fn(ok) == -4      # the unbound engine
        assert fn(L.gen_opts(num_beams=9, use_graph=0)) == -1
        assert fn(L.gen_opts(num_beams=3, max_length=41, use_graph=0)) == -1 and b'max_length' in lib.vitcap_last_error()
    lib.vitcap_engine_destroy(h)


def test_new_symbols_are_exported(L):
    for name in ('vitcap_attn_decode_beam_groups_masked', 'vitcap_engine_decode_beam_masked', 'vitcap_engine_generate_beam_masked'):
        assert name in L.EXPORTS and getattr(L.lib, name) is not None
    from vitcap_amd import ops
    from vitcap_amd.model import ImageCaptioning
    assert callable(ops.attn_decode_beams_masked)
    assert all(callable(getattr(ImageCaptioning, n)) for n in ('caption_regions_beam', 'caption_with_regions_beam', 'refuse_visible_beam'))


# ------------------------------------------------------------------------------------------------ 4: Python and the pipeline
def test_python_beam_calls_refuse_before_touching_the_image(model):
    img = torch.zeros(2, 1)          # never a valid image: every refusal below comes first
    ok = torch.ones(2, 578, dtype=torch.bool)
    boxes = RG.grid_regions(2)
    calls = (lambda nb, **kw: model.generate_beam(img, nb, visible=ok, **kw),
             lambda nb, **kw: model.caption_regions_beam(img, boxes, nb, **kw),
             lambda nb, **kw: model.caption_with_regions_beam(img, boxes, nb, **kw))
    for call in calls:
        for nb in (1, 9, 0):
            with pytest.raises(NotImplementedError, match='num_beams'):
                call(nb)
        for over, name in (({'use_cbs': True}, 'use_cbs'), ({'tag_visible': 5}, 'tag_visible'), ({'do_sample': True}, 'do_sample'),
                           ({'use_graph': True}, 'use_graph'), ({'prefix_ids': torch.tensor([[2000]])}, 'prefix_ids')):
            with pytest.raises(NotImplementedError, match=name):
                call(3, **over)
    for bad in (torch.ones(2, 578), torch.ones(2, 578, dtype=torch.int32)):
        with pytest.raises(ValueError, match='bool or uint8'):
            model.generate_beam(img, 3, visible=bad)
    for bad in (torch.ones(3, 578, dtype=torch.bool), torch.ones(2, 24, 25, dtype=torch.uint8)):
        with pytest.raises(ValueError, match='visible must be'):
            model.generate_beam(img, 3, visible=bad)
    with pytest.raises(ValueError, match='empty box'):
        model.caption_regions_beam(img, torch.tensor([[3, 3, 3, 9]]), 3)
    with pytest.raises(ValueError, match='outside'):
        model.caption_with_regions_beam(img, torch.tensor([[0, 0, 30, 9]]), 3)
    with pytest.raises(ValueError, match='boxes must be'):
        model.caption_regions_beam(img, torch.zeros(3, 2, 4, dtype=torch.int64) + torch.tensor([0, 0, 1, 1]), 3)


def test_the_older_calls_keep_their_refusals(model, L):
    """What tests/test_region_cpu.py pins, restated: the greedy calls refuse num_beams by name, in Python, in the engine and in the
    pipeline."""
    img, ok, boxes = torch.zeros(2, 1), torch.ones(2, 578, dtype=torch.bool), RG.grid_regions(2)
    caps = torch.full((2, 20), 2000, dtype=torch.int64)
    for call in (lambda: model.generate(img, visible=ok, num_beams=2), lambda: model.caption_regions(img, boxes, num_beams=2),
                 lambda: model.generate_multi(img, 2, visible=torch.ones(4, 578, dtype=torch.bool), num_beams=2),
                 lambda: model.score_masked(img, caps, ok, one_pass=False, num_beams=2),
                 lambda: model.caption_with_regions(img, boxes, num_beams=2)):
        with pytest.raises(NotImplementedError, match='num_beams'):
            call()
    h = C.c_void_p()
    assert L.lib.vitcap_engine_create(C.byref(h)) == 0
    buf = (C.c_char * 1024)()
    a = C.c_void_p((C.addressof(buf) + 255) & ~255)
    o = L.gen_opts(num_beams=2, use_graph=0)
    assert L.lib.vitcap_engine_decode_masked(h, 1, C.byref(o), a, 1 << 40, None, 0, a, a, None, None, a, None) == -1 and b'num_beams' in L.lib.vitcap_last_error()
    assert L.lib.vitcap_engine_generate_masked(h, a, 0, 1, C.byref(o), a, 1 << 40, None, 0, a, a, None, None, None, a, None) == -1 and b'num_beams' in L.lib.vitcap_last_error()
    L.lib.vitcap_engine_destroy(h)


def test_pipeline_key_parses_and_refuses():
    from vitcap_amd.pipeline import CaptionUniPipeline
    pl = CaptionUniPipeline(full_expid='E', init_recipe_seed=0, regions=2, regions_beams=3)
    assert int(pl.cfg.regions_beams) == 3 and not CaptionUniPipeline(full_expid='E', init_recipe_seed=0, regions=2).cfg.regions_beams
    pl.check_regions()
    with pytest.raises(ValueError, match='only valid next to'):
        CaptionUniPipeline(full_expid='E', init_recipe_seed=0, regions_beams=3).ensure_predict()
    for k in (1, 9, 0, 2.5, True, -3):
        with pytest.raises(ValueError, match='regions_beams'):
            CaptionUniPipeline(full_expid='E', init_recipe_seed=0, regions=2, regions_beams=k).ensure_predict()
    for kw, name in (({'num_beams': 2}, 'num_beams'), ({'use_cbs': True}, 'use_cbs'), ({'caption_prefix': 'a photo of'}, 'caption_prefix'),
                     ({'tag_visible': 5}, 'tag_visible'), ({'occlusion': 8}, 'occlusion')):
        with pytest.raises(NotImplementedError, match=name):
            CaptionUniPipeline(full_expid='E', init_recipe_seed=0, regions=2, regions_beams=3, **kw).ensure_predict()
    with pytest.raises(NotImplementedError, match='num_beams'):       # pinned: `regions: g` with num_beams > 1 stays refused
        CaptionUniPipeline(full_expid='E', init_recipe_seed=0, regions=2, num_beams=2).ensure_predict()


class _Tok:
    def decode(self, ids, skip_special_tokens=True):
        return ' '.join('w%d' % i for i in ids if i not in (BOS, EOS, PAD))


def test_to_rows_takes_the_n_best_shape():
    ids = torch.tensor([[[[BOS, 5, 6, EOS, PAD], [BOS, 5, EOS, PAD, PAD]], [[BOS, 7, EOS, PAD, PAD], [PAD, PAD, PAD, PAD, PAD]]]])
    lp = torch.tensor([[[0.0, -1.0], [-0.5, -1e5]]])
    rows = RG.to_rows(ids, lp, RG.grid_regions(2)[1:3], _Tok())
    assert len(rows) == 1 and len(rows[0]) == 2
    assert rows[0][0] == {'rect': [192, 0, 384, 192], 'caption': 'w5 w6', 'conf': 1.0,
                          'nbest': [{'caption': 'w5 w6', 'conf': 1.0}, {'caption': 'w5', 'conf': math.exp(-1.0)}]}
    assert rows[0][1]['caption'] == 'w7' and rows[0][1]['nbest'] == [{'caption': 'w7', 'conf': math.exp(-0.5)}]   # the empty slot is left out
    one = RG.to_rows(ids[:, :, :1], lp[:, :, :1], RG.grid_regions(2)[1:3], _Tok())
    assert one == RG.to_rows(ids[:, :, 0], lp[:, :, 0], RG.grid_regions(2)[1:3], _Tok()) and 'nbest' not in one[0][0]
    with pytest.raises(ValueError, match='n-best ids'):
        RG.to_rows(ids, lp[:, :, 0], RG.grid_regions(2)[1:3], _Tok())
    with pytest.raises(ValueError, match='to_rows needs ids'):
        RG.to_rows(ids[0, 0], lp[0, 0], RG.grid_regions(2)[1:3], _Tok())
