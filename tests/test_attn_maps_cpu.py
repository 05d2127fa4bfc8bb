"""Attention maps of given captions: what is decided without a GPU.

The reference fixture (tests/golden/reference_attn.npz, written by tests/golden/make_golden_attn.py from the reference's own
attention_probs) and its invariants; the fp64 restatement of the row definition (tests/attn_maps_ref.py) and the teeth of both
comparators -- the op bound against mutations planted into the restatement, the end-to-end bound against mutations of the fixture;
the host-side refusals of the Python calls and of the engine entry points; the host helpers of vitcap_amd/attnmaps.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import attn_maps_ref as R
from score_request_calls import entry_points

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOS, EOS, PAD = 101, 102, 0
NVIS, LMAX = 578, 20


@pytest.fixture(scope='module')
def L():
    from vitcap_amd import _lib
    return _lib


@pytest.fixture(scope='module')
def model():
    from vitcap_amd.model import ImageCaptioning
    return ImageCaptioning(tie_weights=True, tagemb='cls')


@pytest.fixture(scope='module')
def fixture():
    return dict(np.load(os.path.join(REPO, 'tests', 'golden', 'reference_attn.npz')))


def _caps(rows, max_len=20):
    c = torch.full((rows, max_len), 2000, dtype=torch.int64)
    c[:, 0] = BOS
    c[:, -1] = EOS
    return c


# ------------------------------------------------------------------------------------------------ 1
def test_fixture_invariants(fixture, golden):
    f = fixture
    W = NVIS + LMAX
    assert f['mean'].shape == (2, 4, 4, W) and f['per_head'].shape == (2, 2, 12, W) and f['mean'].dtype == np.float32
    assert f['steps'].tolist() == [1, 5, 10, 19] and f['per_head_steps'].tolist() == [1, 19] and f['per_head_layers'].tolist() == [0, 3]
    assert float(f['tag_mass']) == 0.0                               # the 50 masked tag columns the layout drops hold exactly 0
    assert (f['ids'] == golden[0]['greedy_b2_ids'][:, 0]).all()      # the captions are the greedy golden's
    assert np.abs(f['mean'].astype(np.float64).sum(-1) - 1).max() < 1e-5
    assert np.abs(f['per_head'].astype(np.float64).sum(-1) - 1).max() < 1e-5
    for si, t in enumerate(f['steps']):
        assert (f['mean'][:, si, :, NVIS + t + 1:] == 0).all() and (f['mean'][:, si, :, :NVIS + t + 1] > 0).all()
    for si, t in enumerate(f['per_head_steps']):
        assert (f['per_head'][si, :, :, NVIS + t + 1:] == 0).all()
    # the head mean of the stored per-head rows is the stored head mean (image 0)
    for si, t in enumerate(f['per_head_steps']):
        for li, l in enumerate(f['per_head_layers']):
            want = f['mean'][0, list(f['steps']).index(t), l]
            assert np.abs(f['per_head'][si, li].astype(np.float64).mean(0) - want).max() < 1e-7
    assert os.path.getsize(os.path.join(REPO, 'tests', 'golden', 'reference_attn.npz')) < 200 * 1024


# ------------------------------------------------------------------------------------------------ 2, 3
@pytest.fixture(scope='module')
def planted():
    """(1 image, 3 captions, L = 8), planted peaks, none of the captions ended: inputs, ids, the restatement's maps."""
    q, v = R.make_inputs(1, 3, 8, seed=5, planted=True)
    ids = R.captions(3, 8, seed=1)
    ids[ids == EOS] = 2000
    ids[ids == PAD] = 2001
    return q, v, ids, R.probe_maps_ref(q, v, ids, 1, 3, 8)


def test_restatement_is_the_row_definition(planted):
    q, v, ids, ref = planted
    L_, W = 8, NVIS + 8
    assert tuple(ref.shape) == (3, L_, 12, W) and ref.dtype == torch.float64
    assert (ref[:, 0] == 0).all()
    assert (ref[:, 1:].sum(-1) - 1).abs().max() < 1e-12
    for t in range(1, L_):
        assert (ref[:, t, :, NVIS + t + 1:] == 0).all() and (ref[:, t, :, :NVIS + t + 1] > 0).all()
    # an independent per-row evaluation: plain softmax over the row's own key list, one (caption, position, head) at a time
    x = q.double().view(3, 15, 2304)
    vis = v.double().view(NVIS, 2304)
    for c, t, h in ((0, 1, 0), (1, 4, 1), (2, 7, 2), (2, 5, 3), (1, 7, 11)):
        qq = x[c, L_ + t - 1, h * 64:(h + 1) * 64]
        keys = torch.cat([vis[:, 768 + h * 64:768 + (h + 1) * 64], x[c, :t, 768 + h * 64:768 + (h + 1) * 64],
                          x[c, L_ + t - 1:L_ + t, 768 + h * 64:768 + (h + 1) * 64]])
        want = torch.softmax(keys @ qq * 0.125, 0)
        assert (ref[c, t, h, :NVIS + t + 1] - want).abs().max() < 1e-12
    # the planted peaks dominate their rows by the known gap: head 1 the probe's own key, head 3 token t - 1, head 2 a visual key
    assert ref[0, 4, 1].argmax() == NVIS + 4 and ref[0, 4, 1].max() > 0.5
    assert ref[0, 4, 3].argmax() == NVIS + 3 and ref[0, 4, 3].max() > 0.5
    assert ref[0, 4, 2].argmax() == (37 * 4) % NVIS and ref[0, 4, 2].max() > 0.5
    # ... and the one planted on token key t (head 0) is invisible
    assert ref[0, 4, 0].max() < 0.1


def test_dead_rows_follow_the_first_end_token():
    q, v = R.make_inputs(1, 4, 8, seed=6)
    ids = R.captions(4, 8, seed=2)        # end at 1, at 4, in the last column, none
    ref = R.probe_maps_ref(q, v, ids, 1, 4, 8)
    live = ref.sum((-1, -2)) > 0
    assert live[0].tolist() == [False, True] + [False] * 6
    assert live[1].tolist() == [False] + [True] * 4 + [False] * 3
    assert live[2].tolist() == [False] + [True] * 7 and live[3].tolist() == [False] + [True] * 7
    # a second EOS id ends a caption too
    ids2 = ids.clone()
    ids2[3, 2] = 1012
    live2 = R.probe_maps_ref(q, v, ids2, 1, 4, 8, eos_extra=(1012,)).sum((-1, -2)) > 0
    assert live2[3].tolist() == [False, True, True] + [False] * 5


@pytest.mark.parametrize('mutation', R.MUTATIONS)
def test_op_bound_rejects_planted_mutations(planted, mutation):
    """The comparator and bound of the GPU op test, against the restatement with one deliberate error."""
    q, v, ids, ref = planted
    mut = R.probe_maps_ref(q, v, ids, 1, 3, 8, mutate=mutation)
    n, worst = R.op_violations(mut, ref)
    assert n > 0 and worst > 100, (mutation, n, worst)
    assert R.op_violations(ref.float(), ref)[0] == 0          # fp32 rounding alone passes
    if mutation != 'head_swap':           # the head mean cannot see the head order; everything else it sees
        n, worst = R.op_violations(R.head_mean(mut), R.head_mean(ref))
        assert n > 0 and worst > 100, (mutation, n, worst)


# ------------------------------------------------------------------------------------------------ 4
def test_end_to_end_bound_rejects_fixture_mutations(fixture):
    """The reference's maps of the seeded recipe are not so flat that a misplaced column, head or layer would pass the end-to-end
    bound: each mutation of the fixture misses it by more than a factor of ten, while the fixture itself passes trivially."""
    mean, ph = fixture['mean'], fixture['per_head']
    assert R.rel_metric(mean, mean)[0] == 0

    def roll(x):
        y = x.copy()
        y[..., :NVIS] = np.roll(x[..., :NVIS], 1, -1)
        return y

    assert R.rel_metric(roll(mean), mean)[0] > 10 * R.E2E_BOUND_MEAN
    assert R.rel_metric(roll(ph), ph)[0] > 10 * R.E2E_BOUND_HEAD
    y = ph.copy()
    y[:, :, [0, 1]] = ph[:, :, [1, 0]]                 # heads 0 and 1
    assert R.rel_metric(y, ph)[0] > 10 * R.E2E_BOUND_HEAD
    y = mean.copy()
    y[:, :, [0, 3]] = mean[:, :, [3, 0]]               # layers 0 and 3
    assert R.rel_metric(y, mean)[0] > 10 * R.E2E_BOUND_MEAN
    y = ph.copy()
    y[:, [0, 1]] = ph[:, [1, 0]]                       # the per-head rows hold layers 0 and 3
    assert R.rel_metric(y, ph)[0] > 10 * R.E2E_BOUND_HEAD


# ------------------------------------------------------------------------------------------------ 5
def test_python_calls_refuse_before_touching_the_image(model):
    img = torch.zeros(2, 1)          # never a valid image: every refusal below comes first
    for over, name in (({'num_beams': 2}, 'num_beams'), ({'use_cbs': True}, 'use_cbs'), ({'repetition_penalty': 1.3}, 'repetition_penalty'),
                       ({'tag_visible': 5}, 'tag_visible'), ({'do_sample': True}, 'do_sample')):
        with pytest.raises(NotImplementedError, match=name):
            model.attention_maps(img, _caps(2), **over)
    with pytest.raises(NotImplementedError, match='seqs_per_image'):
        model.attention_maps(img, _caps(66), seqs_per_image=33)
    bad = _caps(2)
    bad[1, 0] = 2000
    with pytest.raises(ValueError, match=r'\[CLS\]'):
        model.attention_maps(img, bad)
    with pytest.raises(ValueError, match='vocabulary'):
        model.attention_maps(img, _caps(2) + 40000)
    with pytest.raises(ValueError):
        model.attention_maps(img, _caps(3))
    for layers in ((), (4,), (-1, 0)):
        with pytest.raises(ValueError, match='layers'):
            model.attention_maps(img, _caps(2), layers=layers)
    assert model._layer_mask((0, 1, 2, 3)) == 15 and model._layer_mask([3]) == 8 and model._layer_mask((1, 1, 2)) == 6
    with pytest.raises(RuntimeError, match='no encoded images'):
        model.attention_maps_encoded(_caps(2))
    for over, name in (({'num_beams': 2}, 'num_beams'), ({'use_cbs': True}, 'use_cbs'), ({'do_sample': True}, 'do_sample')):
        with pytest.raises(NotImplementedError, match=name):
            model.caption_with_maps(img, **over)


def test_engine_explain_entry_points_refuse_without_a_device(L):
    lib = L.lib
    h = C.c_void_p()
    assert lib.vitcap_engine_create(C.byref(h)) == 0 and h.value
    buf = (C.c_char * 1024)()
    a = C.c_void_p((C.addressof(buf) + 255) & ~255)
    text, whole = entry_points(L, h, a, L.SCORE_MAPS, {'maps': 'maps', 'per_head': 'per_head', 'mask': 'layer_mask'},
                               maps=a, per_head=0, mask=15)
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
        assert fn(None, ids=None) == -1 and b'null' in lib.vitcap_last_error()
        assert fn(None, lp=None) == -1 and fn(None, out_ids=None) == -1 and fn(None, sws=None) == -1
        assert fn(L.gen_opts(max_length=41)) == -1 and b'max_length' in lib.vitcap_last_error()
        assert fn(None, maps=None) == -1 and b'maps' in lib.vitcap_last_error()
        for m in (0, 16, -1):
            assert fn(None, mask=m) == -1 and b'layer_mask' in lib.vitcap_last_error()
        for ph in (2, -1):
            assert fn(None, per_head=ph) == -1 and b'per_head' in lib.vitcap_last_error()
        need = lib.vitcap_engine_score_workspace_bytes(1, 1, None)
        assert fn(None, sws_bytes=need - 1) == -3 and b'score workspace' in lib.vitcap_last_error()
        assert fn(None, sws_bytes=need) == -4 and fn(None, sws_bytes=need, per_head=1, mask=8) == -4      # the unbound engine
    lib.vitcap_engine_destroy(h)


def test_probe_maps_launcher_refuses_bad_arguments(L):
    """Every refusal of vitcap_attn_probe_maps comes before anything is enqueued, so it can be met without a device."""
    lib = L.lib
    buf = (C.c_char * 1024)()
    a = C.c_void_p((C.addressof(buf) + 255) & ~255)
    odd = C.c_void_p(a.value + 2)
    f = lambda qkv=a, vis=a, ids=a, out=a, n=1, K=1, S=578, ml=20, ph=0: lib.vitcap_attn_probe_maps(qkv, vis, ids, out, n, K, S, ml, ph, EOS,
                                                                                                   None, 0.125, None)
    for kw, name in (({'S': 577}, b'S_vis'), ({'ml': 41}, b'max_len'), ({'ml': 1}, b'max_len'), ({'K': 33}, b'caps_per_image'),
                     ({'K': 0}, b'caps_per_image'), ({'ph': 2}, b'per_head'), ({'ph': -1}, b'per_head'), ({'qkv': None}, b'qkv_text'),
                     ({'vis': None}, b'vis_qkv'), ({'ids': None}, b'caption_ids'), ({'out': None}, b'out'), ({'qkv': odd}, b'aligned'),
                     ({'vis': odd}, b'aligned'), ({'ids': odd}, b'misaligned'), ({'out': odd}, b'misaligned'), ({'n': 0}, b'n_images')):
        assert f(**kw) == -1, kw
        assert b'attn_probe_maps' in lib.vitcap_last_error() and name in lib.vitcap_last_error(), (kw, lib.vitcap_last_error())


# ------------------------------------------------------------------------------------------------ 6
def test_host_helpers():
    from vitcap_amd import attnmaps as A
    assert (A.N_VIS, A.COL_TAG_CLS, A.COL_ENC_CLS, A.COL_PATCH0, A.COL_TEXT0, A.GRID) == (578, 0, 1, 2, 578, 24)
    assert A.COL_PATCH0 + A.N_PATCH == A.N_VIS and A.width(20) == 598
    m = torch.arange(2 * 3 * 598, dtype=torch.float32).view(2, 3, 598)
    g = A.patch_grid(m)
    assert tuple(g.shape) == (2, 3, 24, 24)
    assert g[1, 2, 0, 0] == m[1, 2, 2] and g[1, 2, 0, 23] == m[1, 2, 25] and g[1, 2, 1, 0] == m[1, 2, 26] and g[1, 2, 23, 23] == m[1, 2, 577]
    assert torch.equal(A.text_mass(m, 20), m[..., 578:].sum(-1)) and tuple(A.text_mass(m, 20).shape) == (2, 3)
    gn = A.patch_grid(m.numpy())                                         # numpy arrays work the same
    assert gn.shape == (2, 3, 24, 24) and gn[0, 1, 5, 7] == m[0, 1, 2 + 5 * 24 + 7]
    assert np.allclose(A.text_mass(m.numpy(), 20), m.numpy()[..., 578:].sum(-1))
    with pytest.raises(ValueError):
        A.text_mass(m, 21)
    with pytest.raises(ValueError):
        A.patch_grid(m[..., :100])
    # on a fixture row: patches + the two cls columns + the text mass make up the row
    f = np.load(os.path.join(REPO, 'tests', 'golden', 'reference_attn.npz'))['mean']
    tot = A.patch_grid(f).sum((-1, -2)) + f[..., 0] + f[..., 1] + A.text_mass(f, 20)
    assert np.abs(tot - 1).max() < 1e-5


def test_pipeline_refuses_what_the_maps_are_not_built_for():
    """`attention_maps` together with beam search, CBS or a caption prefix is refused before a model is built."""
    from vitcap_amd.pipeline import CaptionUniPipeline
    for kw, name in (({'num_beams': 2}, 'num_beams'), ({'use_cbs': True}, 'use_cbs'), ({'caption_prefix': 'a photo of'}, 'caption_prefix')):
        with pytest.raises(NotImplementedError, match=name):
            CaptionUniPipeline(full_expid='E', init_recipe_seed=0, attention_maps=True, **kw).ensure_predict()
    assert CaptionUniPipeline.get_attention_file('a/b.predict.tsv') == 'a/b.predict.attn.tsv'
