"""Occlusion maps of given captions: what is decided without a GPU.

The host helpers of vitcap_amd/occlusion.py (window masks, packing against numpy.packbits, upsampling, rows); the refusals of the
Python calls (raised before a GPU is touched), of the pipeline key, of the two engine entry points (on an engine without weights, with
pointers that are never followed) and of the op-level launcher; the fp64 restatement of the masked attention (tests/occlusion_ref.py)
against its own deliberately wrong variants on planted inputs, and against the rounding-emulated form."""
import ctypes as C

import numpy as np
import pytest
import torch

import occlusion_ref as R
from score_request_calls import entry_points
from vitcap_amd import occlusion as OC

BOS, EOS, PAD = 101, 102, 0


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


# ------------------------------------------------------------------------------------------------ 1: the host helpers
@pytest.mark.parametrize('window,stride,g', [(4, None, 6), (8, None, 3), (24, None, 1), (1, None, 24), (8, 4, 5), (6, 3, 7), (4, 1, 21)])
def test_window_masks(window, stride, g):
    for keep_cls in (True, False):
        m = OC.window_masks(window, stride, keep_cls=keep_cls)
        assert m.dtype == torch.bool and tuple(m.shape) == (g * g, 578)
        assert bool((m[:, :2] == keep_cls).all())
        hidden = ~m[:, 2:].view(g * g, 24, 24)
        assert bool((hidden.sum((1, 2)) == window * window).all())
        s = stride or window
        for n in (0, g - 1, g * g - 1):
            i, j = divmod(n, g)
            want = torch.zeros(24, 24, dtype=torch.bool)
            want[i * s:i * s + window, j * s:j * s + window] = True
            assert torch.equal(hidden[n], want)
        if stride is None:
            assert bool((hidden.sum(0) == 1).all()), 'every patch hidden exactly once at stride == window'
        only = OC.window_masks(window, stride, keep_cls=keep_cls, keep_only=True)
        assert torch.equal(only[:, 2:], ~m[:, 2:]) and torch.equal(only[:, :2], m[:, :2])


def test_window_refusals():
    for w in (0, 25, -1, 2.5, True):
        with pytest.raises(ValueError, match='window must be 1..24'):
            OC.window_masks(w)
    for w, s in ((4, 0), (4, 5), (4, -1), (4, 1.5)):
        with pytest.raises(ValueError, match='stride must be 1..window'):
            OC.window_masks(w, s)
    for w, s in ((5, None), (7, 7), (8, 3), (10, 4)):
        with pytest.raises(ValueError, match=r'\(24 - window\) % stride'):
            OC.window_masks(w, s)
    assert OC.check_window(4) == (4, 4, 6) and OC.check_window(8, 4) == (8, 4, 5) and OC.check_window(24) == (24, 24, 1)


def test_pack_visible_against_packbits():
    g = torch.Generator().manual_seed(5)
    m = torch.rand(11, 578, generator=g) < 0.5
    m[0] = True
    m[1] = False
    m[2] = False
    m[2, 577] = True
    m[3] = False
    m[3, 31] = True           # the sign bit of word 0
    got = OC.pack_visible(m)
    assert got.dtype == torch.int32 and tuple(got.shape) == (11, 19)
    padded = np.zeros((11, 608), dtype=np.uint8)
    padded[:, :578] = m.numpy()
    want = np.packbits(padded, axis=1, bitorder='little').view('<u4')
    assert np.array_equal(got.numpy().view(np.uint32), want)
    assert int(got[3, 0]) == -2 ** 31 and int(got[2, 18]) == 2 and bool((got[1] == 0).all())
    assert np.array_equal(OC.pack_visible(m.to(torch.uint8)).numpy(), got.numpy())
    assert np.array_equal(OC.pack_visible(m.numpy()).numpy(), got.numpy())
    for k in (0, 15, 16, 31, 32, 575, 576, 577):
        one = torch.zeros(1, 578, dtype=torch.bool)
        one[0, k] = True
        w = OC.pack_visible(one).numpy().view(np.uint32)[0]
        assert int(w[k >> 5]) == 1 << (k & 31) and int(w.astype(np.uint64).sum()) == 1 << (k & 31)
    with pytest.raises(ValueError, match='pack_visible'):
        OC.pack_visible(torch.ones(3, 577, dtype=torch.bool))


def test_as_visible():
    grid = torch.zeros(2, 24, 24, dtype=torch.uint8)
    grid[1, 3, 5] = 1
    v = OC.as_visible(grid, 2)
    assert v.dtype == torch.bool and tuple(v.shape) == (2, 578)
    assert bool(v[:, :2].all()) and int(v[0, 2:].sum()) == 0 and int(v[1].sum()) == 3 and bool(v[1, 2 + 3 * 24 + 5])
    flat = torch.rand(2, 578) < 0.5
    assert torch.equal(OC.as_visible(flat, 2), flat)
    for bad in (torch.ones(2, 578), torch.ones(2, 578, dtype=torch.int64)):
        with pytest.raises(ValueError, match='bool or uint8'):
            OC.as_visible(bad, 2)
    for bad in (torch.ones(3, 578, dtype=torch.bool), torch.ones(2, 577, dtype=torch.bool), torch.ones(2, 24, 23, dtype=torch.bool),
                torch.ones(578, dtype=torch.bool)):
        with pytest.raises(ValueError, match='visible must be'):
            OC.as_visible(bad, 2)


def test_upsample():
    d = torch.arange(2 * 3 * 36, dtype=torch.float32).view(2, 3, 6, 6)
    up = OC.upsample(d, 4)
    assert tuple(up.shape) == (2, 3, 24, 24)
    assert torch.equal(up, d.repeat_interleave(4, 2).repeat_interleave(4, 3))       # disjoint windows: each patch takes its window's
    d2 = torch.rand(1, 2, 5, 5, dtype=torch.float64)
    up2 = OC.upsample(d2, 8, 4)
    assert float(up2[0, 1, 0, 0]) == pytest.approx(float(d2[0, 1, 0, 0]))            # the corner: one window
    assert float(up2[0, 1, 5, 9]) == pytest.approx(float((d2[0, 1, 0, 1] + d2[0, 1, 0, 2] + d2[0, 1, 1, 1] + d2[0, 1, 1, 2]) / 4))
    assert float(up2[0, 0, 23, 4]) == pytest.approx(float((d2[0, 0, 4, 0] + d2[0, 0, 4, 1]) / 2))
    with pytest.raises(ValueError, match='upsample'):
        OC.upsample(d, 8)


class _Tok:
    def __init__(self, toks):
        self.ids_to_tokens = toks


def test_to_rows():
    toks = ['w%d' % i for i in range(200)]
    ids = torch.tensor([[[101, 5, 6, 102, 0, 0]], [[101, 7, 8, 9, 10, 102]]])
    drop = torch.arange(2 * 6 * 4, dtype=torch.float32).view(2, 6, 2, 2) / 8
    rows = OC.to_rows(ids, drop, _Tok(toks))
    assert [len(r) for r in rows] == [3, 5]
    assert [rec['word'] for rec in rows[0]] == ['w5', 'w6', 'w102']
    assert rows[1][4] == {'word': 'w102', 'drop': drop[1, 5].tolist()}
    assert rows[0][0]['drop'] == drop[0, 1].tolist()
    assert [rec['word'] for rec in OC.to_rows(ids, drop, _Tok(toks), eos=(102, 6))[0]] == ['w5', 'w6']


# ------------------------------------------------------------------------------------------------ 2: Python refusals
def test_python_calls_refuse_before_touching_the_image(model):
    img = torch.zeros(2, 1)          # never a valid image: every refusal below comes first
    ok = torch.ones(2, 578, dtype=torch.bool)
    for bad in (torch.ones(2, 578), torch.ones(2, 578, dtype=torch.int32)):
        with pytest.raises(ValueError, match='bool or uint8'):
            model.score_masked(img, _caps(2), bad)
    for bad in (torch.ones(3, 578, dtype=torch.bool), torch.ones(2, 576, dtype=torch.bool), torch.ones(2, 24, 25, dtype=torch.uint8),
                torch.ones(4, 24, 24, dtype=torch.bool)):
        with pytest.raises(ValueError, match='visible must be'):
            model.score_masked(img, _caps(2), bad)
    with pytest.raises(ValueError, match='visible must be'):
        model.score_masked(img, _caps(4), ok, seqs_per_image=2)
    for over, name in (({'num_beams': 2}, 'num_beams'), ({'use_cbs': True}, 'use_cbs'), ({'do_sample': True}, 'do_sample'),
                       ({'repetition_penalty': 1.3}, 'repetition_penalty'), ({'tag_visible': 5}, 'tag_visible')):
        with pytest.raises(NotImplementedError, match=name):
            model.score_masked(img, _caps(2), ok, **over)
        with pytest.raises(NotImplementedError, match=name):
            model.occlusion_maps(img, _caps(2), **over)
        with pytest.raises(NotImplementedError, match=name):
            model.visual_gain(img, _caps(2), **over)
    with pytest.raises(NotImplementedError, match='seqs_per_image'):
        model.score_masked(img, _caps(66), torch.ones(66, 578, dtype=torch.bool), seqs_per_image=33)
    bad = _caps(2)
    bad[1, 0] = 2000
    with pytest.raises(ValueError, match=r'\[CLS\]'):
        model.score_masked(img, bad, ok)
    with pytest.raises(ValueError):
        model.occlusion_maps(img, _caps(3))
    for kw, name in (({'window': 0}, 'window must be'), ({'window': 25}, 'window must be'), ({'window': 4, 'stride': 5}, 'stride must be'),
                     ({'window': 4, 'stride': 0}, 'stride must be'), ({'window': 5}, r'\(24 - window\) % stride'),
                     ({'window': 8, 'stride': 3}, r'\(24 - window\) % stride')):
        with pytest.raises(ValueError, match=name):
            model.occlusion_maps(img, _caps(2), **kw)
        with pytest.raises(ValueError, match=name):
            model.occlusion_maps_encoded(_caps(2), **kw)
        with pytest.raises(ValueError, match=name):
            model.caption_with_occlusion(img, **kw)
    for who in (lambda: model.score_masked_encoded(_caps(2), ok), lambda: model.occlusion_maps_encoded(_caps(2))):
        with pytest.raises(RuntimeError, match='no encoded images'):
            who()
    for over, name in (({'num_beams': 2}, 'num_beams'), ({'use_cbs': True}, 'use_cbs'), ({'do_sample': True}, 'do_sample')):
        with pytest.raises(NotImplementedError, match=name):
            model.caption_with_occlusion(img, **over)


def test_pipeline_refuses_what_the_occlusion_maps_are_not_built_for():
    from vitcap_amd.pipeline import CaptionUniPipeline
    for kw, name in (({'num_beams': 2}, 'num_beams'), ({'use_cbs': True}, 'use_cbs'), ({'caption_prefix': 'a photo of'}, 'caption_prefix'),
                     ({'tag_visible': 5}, 'tag_visible'), ({'attention_maps': True}, 'attention_maps'), ({'alternatives': 3}, 'alternatives')):
        with pytest.raises(NotImplementedError, match=name):
            CaptionUniPipeline(full_expid='E', init_recipe_seed=0, occlusion=8, **kw).ensure_predict()
    for w in (25, -2, 5):
        with pytest.raises(ValueError, match='occlusion'):
            CaptionUniPipeline(full_expid='E', init_recipe_seed=0, occlusion=w).ensure_predict()
    assert CaptionUniPipeline.get_occlusion_file('a/b.predict.tsv') == 'a/b.predict.occ.tsv'


# ------------------------------------------------------------------------------------------------ 3: the C entry points
def test_engine_score_masked_entry_points_refuse_without_a_device(L):
    lib = L.lib
    h = C.c_void_p()
    assert lib.vitcap_engine_create(C.byref(h)) == 0 and h.value
    buf = (C.c_char * 1024)()
    a = C.c_void_p((C.addressof(buf) + 255) & ~255)
    text, whole = entry_points(L, h, a, L.SCORE_MASKED, {'mask': 'vis_mask'}, mask=a)
    sp = L.SampleParams(1, 1.0, 0, 1.0, 0)
    refused = ((L.gen_opts(num_beams=2), b'num_beams'),
               (L.gen_opts(use_cbs=1, cbs_states=8, fsm=4096, num_constraints=4096), b'use_cbs'),
               (L.gen_opts(tag_visible=5), b'tag_visible'),
               (L.gen_opts(sampling=sp), b'do_sample'),
               (L.gen_opts(repetition_penalty=1.3), b'repetition_penalty'))
    for fn in (text, whole):
        for o, name in refused:
            assert fn(o) == -1 and name in lib.vitcap_last_error(), name
        for K in (0, 33):
            assert fn(None, K=K) == -1 and b'caps_per_image' in lib.vitcap_last_error()
        assert fn(L.gen_opts(max_length=41)) == -1 and b'max_length' in lib.vitcap_last_error()
        assert fn(None, B=0) == -1 and b'engine_score_masked: bad batch' in lib.vitcap_last_error()
        assert fn(None, mask=None) == -1 and b'engine_score_masked: vis_mask is null' in lib.vitcap_last_error()
        assert fn(None, mask=C.c_void_p(a.value + 2)) == -1 and b'vis_mask is not 4-byte aligned' in lib.vitcap_last_error()
        # the order: options before the batch before the mask before io before the workspace
        assert fn(L.gen_opts(num_beams=2), B=0, mask=None, ids=None) == -1 and b'num_beams' in lib.vitcap_last_error()
        assert fn(None, B=0, mask=None, ids=None) == -1 and b'bad batch' in lib.vitcap_last_error()
        assert fn(None, mask=None, ids=None, sws_bytes=0) == -1 and b'vis_mask' in lib.vitcap_last_error()
        assert fn(None, ids=None, sws_bytes=0) == -1 and b'null caption_ids' in lib.vitcap_last_error()
        assert fn(None, lp=None) == -1 and fn(None, out_ids=None) == -1 and fn(None, sws=None) == -1
        need = lib.vitcap_engine_score_workspace_bytes(1, 1, None)
        assert fn(None, sws_bytes=need - 1) == -3 and b'score workspace' in lib.vitcap_last_error()
        assert fn(None, sws_bytes=need) == -4      # the unbound engine
    lib.vitcap_engine_destroy(h)


def test_attn_text_grid_masked_launcher_refuses_bad_arguments(L):
    """Every refusal of vitcap_attn_text_grid_masked comes before anything is enqueued, so it can be met without a device."""
    lib = L.lib
    buf = (C.c_char * 1024)()
    a = C.c_void_p((C.addressof(buf) + 255) & ~255)

    def f(q=a, vis=a, vt=a, mask=a, out=a, n_img=1, K=1, S=578, ml=20):
        return lib.vitcap_attn_text_grid_masked(q, vis, vt, mask, out, n_img, K, S, ml, 0.125, None)

    for kw, name in (({'mask': None}, b'vis_mask is null'), ({'mask': C.c_void_p(a.value + 1)}, b'vis_mask is not 4-byte aligned'),
                     ({'mask': C.c_void_p(a.value + 2)}, b'vis_mask is not 4-byte aligned'), ({'S': 577}, b'S_vis'), ({'ml': 41}, b'max_len'),
                     ({'ml': 1}, b'max_len'), ({'K': 33}, b'caps_per_image'), ({'K': 0}, b'caps_per_image'), ({'q': None}, b'bad arguments'),
                     ({'out': None}, b'bad arguments'), ({'n_img': 0}, b'bad arguments'), ({'vt': C.c_void_p(a.value + 8)}, b'misaligned')):
        assert f(**kw) == -1, kw
        assert b'attn_text_grid_masked' in lib.vitcap_last_error() and name in lib.vitcap_last_error(), (kw, lib.vitcap_last_error())


def test_new_symbols_are_exported(L):
    for name in ('vitcap_attn_text_grid_masked', 'vitcap_engine_score_req'):
        assert name in L.EXPORTS and getattr(L.lib, name) is not None
    from vitcap_amd import ops
    assert callable(ops.attn_text_grid_masked)


# ------------------------------------------------------------------------------------------------ 4: the restatement and its teeth
@pytest.fixture(scope='module')
def planted():
    n_img, K, L_ = 2, 3, 8
    x, v, visible, want_set = R.planted_inputs(n_img, K, L_, 31)
    ref = R.masked_grid_ref(x, v, visible, n_img, K, L_, emulate=False)
    return n_img, K, L_, x, v, visible, want_set, ref


def test_restatement_moves_exactly_the_planted_slices(planted):
    n_img, K, L_, x, v, visible, want_set, ref = planted
    plain = R.masked_grid_ref(x, v, torch.ones_like(visible), n_img, K, L_, emulate=False)
    got_set, inside, outside = R.moved(ref, plain, L_)
    print('MEASURED planted inputs: smallest planted move %.3f, largest unplanted move %.3e (threshold %.1f)' % (inside, outside, R.MOVE_THRESHOLD))
    assert got_set == want_set and len(want_set) == n_img * K * 4
    assert inside > 2 * R.MOVE_THRESHOLD and outside < R.MOVE_THRESHOLD / 10


@pytest.mark.parametrize('mutate', R.MUTATIONS)
def test_comparator_rejects_each_mutation(planted, mutate):
    """Each deliberately wrong variant misses the attention comparator's bound against the restatement, in fp64 and in the
    rounding-emulated form, while the emulated form itself stays inside it."""
    n_img, K, L_, x, v, visible, want_set, ref = planted
    bad, worst = R.violations(R.masked_grid_ref(x, v, visible, n_img, K, L_, mutate=mutate, emulate=False), ref)
    assert bad > 0 and worst > 0.1, (mutate, bad, worst)
    emu = R.masked_grid_ref(x, v, visible, n_img, K, L_)
    assert R.violations(emu, ref)[0] == 0
    assert R.violations(R.masked_grid_ref(x, v, visible, n_img, K, L_, mutate=mutate), emu)[0] > 0


def test_restatement_all_visible_is_the_unmasked_grid_and_all_hidden_is_text_only():
    """All bits set: the masked restatement equals the unmasked emulation of tests/test_hip_score_onepass.py bit for bit.  All clear:
    the rows attend their own tokens only -- the visual V rows have no influence."""
    n_img, K, L_ = 2, 2, 8
    g = torch.Generator().manual_seed(9)
    x = torch.randn(n_img * K * (2 * L_ - 1), 2304, generator=g).to(torch.bfloat16)
    v = torch.randn(n_img * 578, 2304, generator=g).to(torch.bfloat16)
    ones = torch.ones(n_img * K, 578, dtype=torch.bool)
    from oracle import vitcap_oracle as O
    Rr, NC = 2 * L_ - 1, n_img * K
    xs, vs = x.view(NC, Rr, 2304), v.view(n_img, 578, 2304).repeat_interleave(K, 0)
    Kk = torch.cat([vs[..., 768:1536], xs[..., 768:1536]], 1).float().view(NC, 578 + Rr, 12, 64).transpose(1, 2)
    Vv = torch.cat([vs[..., 1536:], xs[..., 1536:]], 1).float().view(NC, 578 + Rr, 12, 64).transpose(1, 2)
    s = xs[..., :768].float().view(NC, Rr, 12, 64).transpose(1, 2) @ Kk.transpose(-1, -2)
    s[..., 578:].masked_fill_(~R.grid_mask(L_), float('-inf'))
    plain = O.softmax_pv_rounded(s, Vv, O._R(True)).transpose(1, 2).reshape(NC, Rr, 768)
    assert torch.equal(R.masked_grid_ref(x, v, ones, n_img, K, L_), plain)
    hidden = R.masked_grid_ref(x, v, ~ones, n_img, K, L_, emulate=False)
    v2 = v.clone()
    v2[:, 1536:] = 0
    assert torch.equal(R.masked_grid_ref(x, v2, ~ones, n_img, K, L_, emulate=False), hidden)
    assert torch.allclose(hidden[:, 0], x.view(NC, Rr, 2304)[:, 0, 1536:].double())      # token row 0 sees token 0 alone
