"""Region captions: what is decided without a GPU.

The restatement of the masked decode-step attention (tests/region_ref.py) against its own deliberately wrong variants on planted
inputs, and its rounding-emulated form against fp64; the masked greedy loop of the reference against the oracle's golden captions
and the selection conditions of the end-to-end case of tests/test_hip_regions.py (whose reference results live in
tests/golden/region_captions.npz and are recomputed here); the host helpers of vitcap_amd/regions.py; the refusals of the Python
calls (raised before a GPU is touched), of the pipeline key, of the engine entry points (on an engine without weights, with pointers
that are never followed) and of the op-level launcher."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import region_ref as RR
from conftest import GREEDY_MARGIN_FLOOR
from vitcap_amd import regions as RG

BOS, EOS, PAD = 101, 102, 0
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def L():
    from vitcap_amd import _lib
    return _lib


@pytest.fixture(scope='module')
def model():
    from vitcap_amd.model import ImageCaptioning
    return ImageCaptioning(tie_weights=True, tagemb='cls')


def _caps(rows, max_len=20):
    c = torch.full((rows, max_len), 2000, dtype=torch.int64)
    c[:, 0] = BOS
    c[:, -1] = EOS
    return c


# ------------------------------------------------------------------------------------------------ 1: the restatement's teeth
# S_vis at which every head of every row holds a planted key (2 * 12 * 4 <= S - 1); at 33 keys the unplanted heads spread their weight
# over so few keys that the emulation's own bf16 rounding of P reaches the bound against fp64 (measured: 4.4e-3 on two elements)
@pytest.mark.parametrize('spi', [1, 2])
@pytest.mark.parametrize('t', [1, 19])
@pytest.mark.parametrize('S', [129, 578])
def test_comparator_rejects_each_mutation(S, t, spi):
    vis, cache, step, visible = RR.planted_inputs(S, spi, t)
    want = RR.decode_ref(vis, cache, step, t, spi, visible, emulate=False)
    n, worst = RR.violations(RR.decode_ref(vis, cache, step, t, spi, visible), want)
    assert n == 0, 'the rounding-emulated restatement misses the bound against fp64: %d elements, max %.3e' % (n, worst)
    for mutate in RR.MUTATIONS:
        n, worst = RR.violations(RR.decode_ref(vis, cache, step, t, spi, visible, mutate=mutate, emulate=False), want)
        assert n > 100 and worst > 0.5, '%s: only %d elements off, max %.3e' % (mutate, n, worst)
    # and the mask matters at all: with everything visible the planted keys hold their rows
    n, worst = RR.violations(RR.decode_ref(vis, cache, step, t, spi, None, emulate=False), want)
    assert n > 100 and worst > 0.5


def test_restatement_all_visible_is_the_unmasked_reference():
    """With every key visible the restatement is tests/test_hip_attn_decode_kv.py's reference, bit for bit."""
    from test_hip_attn_decode_kv import _reference
    for S, t, spi in ((33, 2, 1), (578, 19, 2)):
        vis, cache, step = RR.random_inputs(S, spi, t)
        assert torch.equal(RR.decode_ref(vis, cache, step, t, spi), _reference(vis, cache, step, t, spi))


def test_mask_kinds_and_packing():
    from vitcap_amd.occlusion import pack_visible
    assert RR.kinds_for(33) == ('random', 'all_hidden', 'only_0', 'only_last', 'bit_31', 'bit_last')
    assert RR.kinds_for(578) == RR.MASK_KINDS
    m = RR.masks_by_kind(11, 578, 3)
    assert torch.equal(RR.pack_bits(m), pack_visible(m))
    hi = RR.pack_bits(m, words=20, high_bits=True)
    assert tuple(hi.shape) == (11, 20) and bool((hi[:, 19] == -1).all()) and torch.equal(hi[:, :18], pack_visible(m)[:, :18])
    assert not bool(m[1].any()) and int(m[2].sum()) == 1 and bool(m[2, 0]) and bool(m[3, 577]) and not bool(m[4, 128:256].any())


# ------------------------------------------------------------------------------------------------ 2: the end-to-end reference
def test_masked_greedy_with_everything_visible_is_the_golden_caption(sd_t, golden):
    """greedy_as_written_masked with all 578 keys visible reproduces the reference's own greedy caption of the golden image, its
    log-prob and its margins."""
    from vitcap_amd import weights as W
    vec, _ = golden
    img = torch.from_numpy(W.gen_image_batch(1, 1234))
    with torch.no_grad():
        ids, lp, margins, _, _ = RR.greedy_as_written_masked(sd_t, img, torch.ones(1, 578, dtype=torch.bool), 20)
    assert ids[0].tolist() == vec['greedy_b1_ids'][0, 0].tolist()
    assert abs(float(lp[0]) - float(vec['greedy_b1_logprobs'][0, 0])) < 1e-4
    want = torch.from_numpy(vec['greedy_b1_margins'][0])
    live = torch.isfinite(margins[0])
    assert float((margins[0][live] - want[live]).abs().max()) < 1e-3


def test_the_end_to_end_case_is_decidable_in_the_reference_alone(sd_t):
    """The case of tests/test_hip_regions.py test 3 (two images, two masks each: a 6 x 6 region with the cls tokens, and nothing),
    recomputed: the committed results are the reference's; at least 3 of the 4 captions have every margin above the bf16 noise floor
    and at least 2 differ from the same image's unmasked caption; the greedy loop's score is token_logprobs_as_written's."""
    case = RR.build_case(sd_t)
    gold = np.load(os.path.join(HERE, 'golden', RR.CASE_FILE))
    assert sorted(gold.files) == sorted(case)
    for k in case:
        if case[k].dtype.kind == 'i':
            assert np.array_equal(case[k], gold[k]), k
        else:
            assert np.allclose(case[k], gold[k], rtol=0, atol=1e-4), k
    margins, ids = case['margins'], case['ids']
    clear = (margins > GREEDY_MARGIN_FLOOR).all(-1)                    # (2 images, 2 masks)
    assert int(clear.sum()) >= 3, margins.min(-1)
    differ = (ids != case['unmasked_ids'][:, None]).any(-1)
    assert int(differ.sum()) >= 2
    assert np.allclose(case['greedy_lp'], case['seq_lp'], rtol=0, atol=1e-5)
    print('MEASURED smallest margin per caption', margins.min(-1).tolist(), 'captions that differ from the unmasked one', differ.tolist())


# ------------------------------------------------------------------------------------------------ 3: the host helpers
def test_box_masks_and_grid_regions():
    from vitcap_amd.occlusion import window_masks
    for g in (1, 2, 3, 4, 6, 8, 12, 24):
        boxes = RG.grid_regions(g)
        assert tuple(boxes.shape) == (g * g, 4) and boxes.dtype == torch.int64
        m = RG.box_masks(boxes)
        assert tuple(m.shape) == (g * g, 578) and m.dtype == torch.bool and bool(m[:, :2].all())
        assert bool((m[:, 2:].sum(0) == 1).all())                      # every patch in exactly one tile
        assert torch.equal(m, window_masks(24 // g, keep_only=True))   # the occlusion helper's keep_only windows
        assert not bool(RG.box_masks(boxes, keep_cls=False)[:, :2].any())
    m = RG.box_masks(torch.tensor([[1, 2, 3, 5]]))[0, 2:].view(24, 24)
    assert int(m.sum()) == 6 and bool(m[1:3, 2:5].all())
    vis, boxes = RG.region_masks(torch.tensor([[0, 0, 24, 24], [23, 23, 24, 24]]), 3)
    assert tuple(vis.shape) == (3, 2, 578) and tuple(boxes.shape) == (3, 2, 4) and bool(vis[:, 0].all()) and int(vis[1, 1].sum()) == 3
    grids = torch.zeros(2, 3, 24, 24, dtype=torch.bool)
    grids[1, 2, 5, 7] = True
    vis, boxes = RG.region_masks(grids, 2, keep_cls=False)
    assert boxes is None and int(vis.sum()) == 1 and bool(vis[1, 2, 2 + 5 * 24 + 7])


def test_region_refusals():
    for g in (0, 5, 7, 48, -2, 2.5, True):
        with pytest.raises(ValueError, match='divisor of 24'):
            RG.grid_regions(g)
    for bad in ([[0, 0, 0, 4]], [[4, 0, 4, 4]], [[5, 5, 3, 8]]):
        with pytest.raises(ValueError, match='empty box'):
            RG.box_masks(torch.tensor(bad))
    for bad in ([[-1, 0, 4, 4]], [[0, 0, 25, 4]], [[0, 20, 4, 26]]):
        with pytest.raises(ValueError, match='outside the 24 x 24'):
            RG.box_masks(torch.tensor(bad))
    for bad in (torch.zeros(3, 5, dtype=torch.int64), torch.zeros(0, 4, dtype=torch.int64), torch.tensor(3)):
        with pytest.raises(ValueError, match=r'\(\.\.\., 4\)'):
            RG.box_masks(bad)
    with pytest.raises(ValueError, match='integers'):
        RG.box_masks(torch.tensor([[0.0, 0.0, 4.0, 4.0]]))
    with pytest.raises(ValueError, match=r'shape \(R, 4\)'):
        RG.box_masks(torch.zeros(2, 2, 4, dtype=torch.int64) + torch.tensor([0, 0, 1, 1]))
    with pytest.raises(ValueError, match='boxes must be'):
        RG.region_masks(torch.tensor([[[0, 0, 1, 1]]] * 3), 2)
    with pytest.raises(ValueError, match='grids must be'):
        RG.region_masks(torch.zeros(2, 1, 24, 23, dtype=torch.bool), 2)


class _Tok:
    def decode(self, ids, skip_special_tokens=True):
        return ' '.join('w%d' % i for i in ids if i not in (BOS, EOS, PAD))


def test_to_rows():
    ids = torch.tensor([[[BOS, 5, 6, EOS, PAD], [BOS, 7, EOS, PAD, PAD]]])
    rows = RG.to_rows(ids, torch.tensor([[0.0, -1.0]]), RG.grid_regions(2)[1:3], _Tok())
    assert len(rows) == 1 and len(rows[0]) == 2
    assert rows[0][0] == {'rect': [192, 0, 384, 192], 'caption': 'w5 w6', 'conf': 1.0}
    assert rows[0][1]['rect'] == [0, 192, 192, 384] and rows[0][1]['caption'] == 'w7' and abs(rows[0][1]['conf'] - np.exp(-1.0)) < 1e-12
    with pytest.raises(ValueError, match='to_rows needs boxes'):
        RG.to_rows(ids, torch.zeros(1, 2), RG.grid_regions(2), _Tok())


# ------------------------------------------------------------------------------------------------ 4: Python and pipeline refusals
def test_python_calls_refuse_before_touching_the_image(model):
    img = torch.zeros(2, 1)          # never a valid image: every refusal below comes first
    ok = torch.ones(2, 578, dtype=torch.bool)
    boxes = RG.grid_regions(2)
    for over, name in (({'num_beams': 2}, 'num_beams'), ({'use_cbs': True}, 'use_cbs'), ({'tag_visible': 5}, 'tag_visible')):
        with pytest.raises(NotImplementedError, match=name):
            model.generate(img, visible=ok, **over)
        with pytest.raises(NotImplementedError, match=name):
            model.generate_multi(img, 2, visible=torch.ones(4, 578, dtype=torch.bool), **over)
        with pytest.raises(NotImplementedError, match=name):
            model.score_masked(img, _caps(2), ok, one_pass=False, **over)
        with pytest.raises(NotImplementedError, match=name):
            model.caption_regions(img, boxes, **over)
        with pytest.raises(NotImplementedError, match=name):
            model.caption_with_regions(img, boxes, **over)
    with pytest.raises(NotImplementedError, match='do_sample'):
        model.caption_regions(img, boxes, do_sample=True)
    for bad in (torch.ones(2, 578), torch.ones(2, 578, dtype=torch.int32)):
        with pytest.raises(ValueError, match='bool or uint8'):
            model.generate(img, visible=bad)
    for bad in (torch.ones(3, 578, dtype=torch.bool), torch.ones(2, 24, 25, dtype=torch.uint8)):
        with pytest.raises(ValueError, match='visible must be'):
            model.generate(img, visible=bad)
        with pytest.raises(ValueError, match='visible must be'):
            model.score_masked(img, _caps(2), bad, one_pass=False)
    with pytest.raises(ValueError, match='visible must be'):
        model.generate_multi(img, 3, visible=ok)                       # one row per sequence: 6
    with pytest.raises(ValueError, match='empty box'):
        model.caption_regions(img, torch.tensor([[3, 3, 3, 9]]))
    with pytest.raises(ValueError, match='outside'):
        model.caption_with_regions(img, torch.tensor([[0, 0, 30, 9]]))
    with pytest.raises(ValueError, match='boxes must be'):
        model.caption_regions(img, torch.zeros(3, 2, 4, dtype=torch.int64) + torch.tensor([0, 0, 1, 1]))
    with pytest.raises(RuntimeError, match='no encoded images'):
        model.caption_regions_encoded(boxes)


def test_as_visible_keep_cls():
    from vitcap_amd.occlusion import as_visible
    grid = torch.zeros(2, 24, 24, dtype=torch.bool)
    assert bool(as_visible(grid, 2)[:, :2].all()) and not bool(as_visible(grid, 2, keep_cls=False).any())


def test_pipeline_key_parses_and_refuses():
    from vitcap_amd.pipeline import CaptionUniPipeline
    pl = CaptionUniPipeline(full_expid='E', init_recipe_seed=0, regions=2)
    assert int(pl.cfg.regions) == 2 and not CaptionUniPipeline(full_expid='E', init_recipe_seed=0).cfg.regions
    pl.check_regions()
    for kw, name in (({'num_beams': 2}, 'num_beams'), ({'use_cbs': True}, 'use_cbs'), ({'caption_prefix': 'a photo of'}, 'caption_prefix'),
                     ({'tag_visible': 5}, 'tag_visible'), ({'attention_maps': True}, 'attention_maps'), ({'alternatives': 3}, 'alternatives'),
                     ({'occlusion': 8}, 'occlusion')):
        with pytest.raises(NotImplementedError, match=name):
            CaptionUniPipeline(full_expid='E', init_recipe_seed=0, regions=2, **kw).ensure_predict()
    for g in (5, -2, 48):
        with pytest.raises(ValueError, match='regions'):
            CaptionUniPipeline(full_expid='E', init_recipe_seed=0, regions=g).ensure_predict()
    assert CaptionUniPipeline.get_regions_file('a/b.predict.tsv') == 'a/b.predict.regions.tsv'


# ------------------------------------------------------------------------------------------------ 5: the C entry points
def test_engine_masked_entry_points_refuse_without_a_device(L):
    """vitcap_engine_decode_masked / vitcap_engine_generate_masked on an engine without weights: every refused option returns
    VITCAP_EINVAL with its name before anything else is looked at; an accepted call gets as far as the unbound engine."""
    lib = L.lib
    h = C.c_void_p()
    assert lib.vitcap_engine_create(C.byref(h)) == 0 and h.value
    buf = (C.c_char * 1024)()
    a = C.c_void_p((C.addressof(buf) + 255) & ~255)

    def decode(o, mask=a, B=1):
        return lib.vitcap_engine_decode_masked(h, B, C.byref(o) if o is not None else None, a, 1 << 40, None, 0, a, a, None, None, mask, None)

    def generate(o, mask=a, B=1):
        return lib.vitcap_engine_generate_masked(h, a, 0, B, C.byref(o) if o is not None else None, a, 1 << 40, None, 0, a, a, None, None,
                                                 None, mask, None)

    refused = ((L.gen_opts(num_beams=2, use_graph=0), b'num_beams'),
               (L.gen_opts(use_cbs=1, cbs_states=8, fsm=4096, num_constraints=4096, use_graph=0), b'use_cbs'),
               (L.gen_opts(tag_visible=5, use_graph=0), b'tag_visible'),
               (L.gen_opts(use_graph=1), b'use_graph'))
    ok = L.gen_opts(use_graph=0)
    for fn in (decode, generate):
        for o, name in refused:
            assert fn(o) == -1 and name in lib.vitcap_last_error() and b'masked decoding' in lib.vitcap_last_error(), name
        assert fn(ok, mask=None) == -1 and b'vis_mask is null' in lib.vitcap_last_error()
        assert fn(ok, mask=C.c_void_p(a.value + 2)) == -1 and b'vis_mask is not 4-byte aligned' in lib.vitcap_last_error()
        assert fn(L.gen_opts(max_length=41, use_graph=0)) == -1 and b'max_length' in lib.vitcap_last_error()
        assert fn(ok, B=0) == -1 and b'bad batch' in lib.vitcap_last_error()
        assert fn(ok) == -4      # the unbound engine
    lib.vitcap_engine_destroy(h)


def test_attn_decode_step_masked_launcher_refuses_bad_arguments(L):
    """Every refusal of vitcap_attn_decode_step_masked comes before anything is enqueued, so it can be met without a device."""
    lib = L.lib
    buf = (C.c_char * 1024)()
    a = C.c_void_p((C.addressof(buf) + 255) & ~255)

    def f(q=a, vis=a, cache=a, out=a, B=1, S=578, t=1, ml=20, spi=1, mask=a, words=19):
        return lib.vitcap_attn_decode_step_masked(q, vis, cache, out, B, S, t, ml, spi, 0.125, mask, words, None)

    for kw, name in (({'mask': None}, b'vis_mask is null'), ({'mask': C.c_void_p(a.value + 1)}, b'vis_mask is not 4-byte aligned'),
                     ({'mask': C.c_void_p(a.value + 2)}, b'vis_mask is not 4-byte aligned'), ({'words': 18}, b'mask_words'),
                     ({'S': 33, 'words': 1}, b'mask_words'), ({'words': 0}, b'mask_words'), ({'t': 0}, b'out of range'),
                     ({'t': 20}, b'out of range'), ({'S': 703, 'words': 22}, b'out of range'), ({'S': 0}, b'out of range'),
                     ({'B': 3, 'spi': 2}, b'seq_per_image'), ({'q': None}, b'bad arguments'), ({'out': None}, b'bad arguments'),
                     ({'B': 0}, b'bad arguments')):
        assert f(**kw) == -1, kw
        assert b'attn_decode_masked' in lib.vitcap_last_error() and name in lib.vitcap_last_error(), (kw, lib.vitcap_last_error())


def test_new_symbols_are_exported(L):
    for name in ('vitcap_attn_decode_step_masked', 'vitcap_engine_decode_masked', 'vitcap_engine_generate_masked'):
        assert name in L.EXPORTS and getattr(L.lib, name) is not None
    from vitcap_amd import ops
    assert callable(ops.attn_decode_step_masked)
