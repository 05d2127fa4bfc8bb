"""Token alternatives of given captions: what is decided without a GPU.

The fp64 restatement of the row rule (tests/alternatives_ref.py) against independent torch formulas -- torch.sort(stable=True) on -x,
log_softmax, -(p log p).sum() -- on random and planted rows; the host helpers of vitcap_amd/alternatives.py; the refusals of the
Python calls (raised before a GPU is touched), of the two engine entry points (on an engine without weights, with pointers that are
never followed) and of the op-level launcher; the exported symbols."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import alternatives_ref as R
from score_request_calls import entry_points

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


# ------------------------------------------------------------------------------------------------ 1: the restatement
def _torch_row(x, f, k):
    """The same quantities from formulas that share nothing with the restatement."""
    xt = torch.from_numpy(np.asarray(x, dtype=np.float32))
    _, idx = torch.sort(-xt, stable=True)              # descending, ties in index order; -(-0.0) == +0.0 compare equal
    lsm = torch.log_softmax(xt.double(), -1)
    p = lsm.exp()
    plogp = torch.where(p > 0, p * lsm, torch.zeros_like(p))
    return idx[:k].numpy(), lsm[idx[:k]].numpy(), int((idx == f).nonzero()[0, 0]), float(-plogp.sum()), float(lsm[f])


@pytest.mark.parametrize('V', [16, 1000, 1025, 30522])
def test_restatement_against_torch_formulas(V):
    k = min(16, V)
    rows, fs = R.planted_rows(V, seed=5 + V, ld=V + 3)
    rng = np.random.RandomState(V)
    rand = (rng.randn(4, V) * 3.0).astype(np.float32)
    cases = [(R.PLANTED[i], rows[i, :V], int(fs[i])) for i in range(8)] + [('rand%d' % i, rand[i], int(rng.randint(0, V))) for i in range(4)]
    for name, x, f in cases:
        w = R.row_ref(x, f, k)
        ids, lp, rank, ent, lp_f = _torch_row(x, f, k)
        assert w['ids'].tolist() == ids.tolist(), name
        assert w['rank'] == rank, name
        assert np.abs(w['lp'] - lp).max() < 1e-9 and abs(w['lp_f'] - lp_f) < 1e-9, name
        assert abs(w['entropy'] - ent) < 1e-9, (name, w['entropy'], ent)
        assert w['lp'][0] == -math.log(np.where(x.astype(np.float64) - x.max() < R.EXPF_ZERO, 0, np.exp(x.astype(np.float64) - x.max())).sum()), name
        assert (w['rank'] == 0) == (int(w['ids'][0]) == f), name


def test_planted_rows_are_what_they_claim():
    V = 30522
    rows, fs = R.planted_rows(V, seed=1, ld=30592)
    assert (rows[:, V:] == 1e9).all() and not (fs == EOS).any()
    w = {n: R.row_ref(rows[i, :V], int(fs[i]), 16) for i, n in enumerate(R.PLANTED)}
    assert w['argmax']['rank'] == 0 and w['argmax']['ids'][0] == fs[0]
    assert w['worst']['rank'] == V - 1
    assert w['tie_lower']['rank'] == 1 and w['tie_lower']['ids'][:2].tolist() == [3, 900]
    assert w['tie_higher']['rank'] == 0 and w['tie_higher']['ids'][:2].tolist() == [3, 900]
    assert w['zeros']['ids'][:2].tolist() == [3, 900] and w['zeros']['rank'] == 1      # -0.0 at 3 before +0.0 at 900: the index decides
    assert np.signbit(rows[4, 3]) and not np.signbit(rows[4, 900])
    assert w['all_equal']['rank'] == V // 2 and abs(w['all_equal']['entropy'] - math.log(V)) < 1e-12
    assert w['all_equal']['ids'].tolist() == list(range(16))
    assert w['dominated']['entropy'] == 0.0 and w['dominated']['lp'][0] == 0.0 and w['dominated']['ent_tol'] == 0.0
    assert w['dominated']['rank'] > 0 and -130 < w['dominated']['lp_f'] < -110


def test_live_rows_scored_token_and_ranges():
    ids = np.full((5, 6), 2000, np.int64)
    ids[:, 0] = BOS
    ids[0, 2] = EOS               # ends at 2
    ids[1, 3] = 1012              # ends at 3 on a second EOS id only
    ids[2, 5] = EOS               # the max-length rule's [SEP]
    ids[3, 5] = EOS
    ids[4, 2] = 40000             # outside the vocabulary: the argmax is scored
    live = R.live_rows(ids, eos_extra=(1012,))
    assert live[0].tolist() == [False, True, True, False, False, False]
    assert live[1].tolist() == [False, True, True, True, False, False]
    assert R.live_rows(ids)[1].tolist() == [False] + [True] * 5
    assert live[2].tolist() == [False] + [True] * 5
    V = 3000
    logits = (np.random.RandomState(3).randn(25, V) * 2).astype(np.float32)
    last = np.array([-1, -1, 77, -1, -1])
    w = R.alternatives_ref(logits, V, ids, 4, last_tok=last, eos_extra=(1012,))
    amax = logits.argmax(1).reshape(5, 5)
    assert w['covered'][:, 1:].all() and not w['covered'][:, 0].any()
    assert w['f'][2, 5] == 77 and w['f'][3, 5] == amax[3, 4] and w['f'][4, 2] == amax[4, 1] and w['f'][4, 1] == 2000
    assert w['rank'][3, 5] == 0 and w['rank'][4, 2] == 0
    dead = ~w['live']
    assert (w['ids'][dead] == -1).all() and (w['rank'][dead] == -1).all() and (w['lp'][dead] == 0).all() and (w['entropy'][dead] == 0).all()
    # a row range that starts and ends inside captions: only its positions are covered, with the values of the whole call
    part = R.alternatives_ref(logits[7:18], V, ids, 4, rows0=7, last_tok=last, eos_extra=(1012,))
    assert int(part['covered'].sum()) == 11 and part['covered'][1, 3] and not part['covered'][1, 2] and part['covered'][3, 3] and not part['covered'][3, 4]
    c = part['covered']
    assert (part['ids'][c] == w['ids'][c]).all() and (part['rank'][c] == w['rank'][c]).all() and (part['entropy'][c] == w['entropy'][c]).all()
    assert (part['ids'][~c] == -1).all()


# ------------------------------------------------------------------------------------------------ 2: host helpers
class _Tok:
    ids_to_tokens = ['w%d' % i for i in range(50)]


def _alts():
    from vitcap_amd.alternatives import Alternatives
    ids = torch.tensor([[[-1, -1], [4, 7], [9, 4], [-1, -1]], [[-1, -1], [1, 2], [3, 5], [6, 8]]], dtype=torch.int32)
    lp = torch.tensor([[[0, 0], [-0.1, -2.5], [-0.5, -1.0], [0, 0]], [[0, 0], [-0.2, -3.0], [-0.3, -2.0], [-0.7, -0.9]]])
    rank = torch.tensor([[-1, 0, 1, -1], [-1, 0, 7, 1]], dtype=torch.int32)
    ent = torch.tensor([[0, 0.5, 1.5, 0], [0, 0.25, 2.0, 1.25]])
    tok_lp = torch.tensor([[0, -0.1, -1.0, 0], [0, -0.2, -6.0, -0.9]])
    return Alternatives(ids, lp, rank, ent), tok_lp


def test_host_helpers():
    from vitcap_amd import alternatives as A
    alts, tok_lp = _alts()
    assert A.K_MAX == 16 and A.Alternatives._fields == ('ids', 'logprobs', 'rank', 'entropy')
    words = A.to_words(_Tok, alts, 0)
    assert words[0] == [] and words[3] == [] and [w for w, _ in words[1]] == ['w4', 'w7'] and [w for w, _ in words[2]] == ['w9', 'w4']
    assert words[1][1][1] == pytest.approx(-2.5)
    s = A.summary(tok_lp, alts.rank, alts.ids, alts.entropy)
    assert s['positions'] == 5
    assert s['perplexity'] == pytest.approx(math.exp((0.1 + 1.0 + 0.2 + 6.0 + 0.9) / 5))
    assert s['top1'] == pytest.approx(2 / 5) and s['top5'] == pytest.approx(4 / 5) and s['entropy'] == pytest.approx(5.5 / 5)
    assert A.summary(tok_lp, alts.rank, alts.ids)['entropy'] is None
    sn = A.summary(tok_lp.numpy(), alts.rank.numpy(), alts.ids.numpy(), alts.entropy.numpy())       # numpy arrays work the same
    assert sn['perplexity'] == pytest.approx(s['perplexity']) and sn['top5'] == s['top5']
    with pytest.raises(ValueError, match='same positions'):
        A.summary(tok_lp[:, :3], alts.rank, alts.ids)
    with pytest.raises(ValueError, match='no live position'):
        A.summary(tok_lp[:1, :1], alts.rank[:1, :1], alts.ids[:1, :1])
    u = A.uncertain(alts, tok_lp, 0.4)
    assert [(r, t, i) for r, t, _, i in u] == [(0, 2, 9), (1, 2, 3)] and u[0][2] == pytest.approx(0.5) and u[1][2] == pytest.approx(5.7)
    assert [(r, t) for r, t, _, _ in A.uncertain(alts, tok_lp, 0.1)] == [(0, 2), (1, 2), (1, 3)]
    assert A.uncertain(alts, tok_lp, 10.0) == []
    for bad in (0, 17, -1, 2.5, True):
        with pytest.raises(ValueError, match='k must be 1..16'):
            A.check_k(bad)
    assert A.check_k(16) == 16 and A.check_k(1) == 1


# ------------------------------------------------------------------------------------------------ 3: Python refusals
def test_python_calls_refuse_before_touching_the_image(model):
    img = torch.zeros(2, 1)          # never a valid image: every refusal below comes first
    for k in (0, 17):
        with pytest.raises(ValueError, match='k must be 1..16'):
            model.alternatives(img, _caps(2), k=k)
        with pytest.raises(ValueError, match='k must be 1..16'):
            model.alternatives_encoded(_caps(2), k=k)
        with pytest.raises(ValueError, match='k must be 1..16'):
            model.caption_with_alternatives(img, k=k)
    for over, name in (({'num_beams': 2}, 'num_beams'), ({'use_cbs': True}, 'use_cbs'), ({'do_sample': True}, 'do_sample'),
                       ({'repetition_penalty': 1.3}, 'repetition_penalty'), ({'tag_visible': 5}, 'tag_visible')):
        with pytest.raises(NotImplementedError, match=name):
            model.alternatives(img, _caps(2), **over)
    with pytest.raises(NotImplementedError, match='seqs_per_image'):
        model.alternatives(img, _caps(66), seqs_per_image=33)
    bad = _caps(2)
    bad[1, 0] = 2000
    with pytest.raises(ValueError, match=r'\[CLS\]'):
        model.alternatives(img, bad)
    with pytest.raises(ValueError):
        model.alternatives(img, _caps(3))
    with pytest.raises(RuntimeError, match='no encoded images'):
        model.alternatives_encoded(_caps(2))
    for over, name in (({'num_beams': 2}, 'num_beams'), ({'use_cbs': True}, 'use_cbs'), ({'do_sample': True}, 'do_sample')):
        with pytest.raises(NotImplementedError, match=name):
            model.caption_with_alternatives(img, **over)


def test_pipeline_refuses_what_the_alternatives_are_not_built_for():
    from vitcap_amd.pipeline import CaptionUniPipeline
    for kw, name in (({'num_beams': 2}, 'num_beams'), ({'use_cbs': True}, 'use_cbs'), ({'caption_prefix': 'a photo of'}, 'caption_prefix'),
                     ({'tag_visible': 5}, 'tag_visible'), ({'attention_maps': True}, 'attention_maps')):
        with pytest.raises(NotImplementedError, match=name):
            CaptionUniPipeline(full_expid='E', init_recipe_seed=0, alternatives=3, **kw).ensure_predict()
    for k in (17, -2):
        with pytest.raises(ValueError, match='k must be 1..16'):
            CaptionUniPipeline(full_expid='E', init_recipe_seed=0, alternatives=k).ensure_predict()
    assert CaptionUniPipeline.get_alternatives_file('a/b.predict.tsv') == 'a/b.predict.alt.tsv'


# ------------------------------------------------------------------------------------------------ 4: the C entry points
def test_engine_alternatives_entry_points_refuse_without_a_device(L):
    lib = L.lib
    h = C.c_void_p()
    assert lib.vitcap_engine_create(C.byref(h)) == 0 and h.value
    buf = (C.c_char * 1024)()
    a = C.c_void_p((C.addressof(buf) + 255) & ~255)
    text, whole = entry_points(L, h, a, L.SCORE_ALTS, {'k': 'k', 'ai': 'alt_ids', 'al': 'alt_lp', 'rk': 'rank', 'en': 'entropy'},
                               k=5, ai=a, al=a, rk=a, en=a)
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
        assert fn(None, B=0) == -1 and b'engine_alternatives: bad batch' in lib.vitcap_last_error()
        for k in (0, 17, -3):
            assert fn(None, k=k) == -1 and b'k must be 1..16' in lib.vitcap_last_error()
        for kw in ({'ai': None}, {'al': None}, {'rk': None}, {'en': None}):
            assert fn(None, **kw) == -1 and b'engine_alternatives: null' in lib.vitcap_last_error(), kw
        # the order: options before the batch before k before io before the workspace
        assert fn(L.gen_opts(num_beams=2), B=0, k=0, ids=None) == -1 and b'num_beams' in lib.vitcap_last_error()
        assert fn(None, B=0, k=0, ids=None) == -1 and b'bad batch' in lib.vitcap_last_error()
        assert fn(None, k=0, ids=None, sws_bytes=0) == -1 and b'k must be' in lib.vitcap_last_error()
        assert fn(None, ids=None, sws_bytes=0) == -1 and b'null caption_ids' in lib.vitcap_last_error()
        assert fn(None, lp=None) == -1 and fn(None, out_ids=None) == -1 and fn(None, sws=None) == -1
        need = lib.vitcap_engine_score_workspace_bytes(1, 1, None)
        assert fn(None, sws_bytes=need - 1) == -3 and b'score workspace' in lib.vitcap_last_error()
        assert fn(None, sws_bytes=need) == -4 and fn(None, sws_bytes=need, k=16) == -4      # the unbound engine
    lib.vitcap_engine_destroy(h)


def test_score_rows_alts_launcher_refuses_bad_arguments(L):
    """Every refusal of vitcap_score_rows_alts comes before anything is enqueued, so it can be met without a device."""
    lib = L.lib
    buf = (C.c_char * 1024)()
    a = C.c_void_p((C.addressof(buf) + 255) & ~255)

    def f(logits=a, ldl=30592, V=30522, ids=a, rows0=0, n_rows=1, n_caps=2, ml=20, k=5, ai=a, al=a, rk=a, en=a):
        return lib.vitcap_score_rows_alts(logits, ldl, V, ids, None, rows0, n_rows, n_caps, ml, EOS, None, PAD, k, ai, al, rk, en, None)

    for kw, name in (({'logits': None}, b'null'), ({'ids': None}, b'null'), ({'ai': None}, b'null'), ({'al': None}, b'null'),
                     ({'rk': None}, b'null'), ({'en': None}, b'null'), ({'k': 0}, b'k must be 1..16'), ({'k': 17}, b'k must be 1..16'),
                     ({'V': 4, 'ldl': 4}, b'bad sizes'), ({'V': 32769, 'ldl': 32769}, b'bad sizes'), ({'ldl': 30521}, b'bad sizes'),
                     ({'ml': 41}, b'bad sizes'), ({'ml': 1}, b'bad sizes'), ({'n_caps': 0}, b'bad sizes'), ({'rows0': -1}, b'outside'),
                     ({'n_rows': 0}, b'outside'), ({'rows0': 0, 'n_rows': 39}, b'outside'), ({'rows0': 38, 'n_rows': 1}, b'outside')):
        assert f(**kw) == -1, kw
        assert b'score_rows_alts' in lib.vitcap_last_error() and name in lib.vitcap_last_error(), (kw, lib.vitcap_last_error())


def test_new_symbols_are_exported(L):
    for name in ('vitcap_score_rows_alts', 'vitcap_engine_score_req'):
        assert name in L.EXPORTS and getattr(L.lib, name) is not None
    from vitcap_amd import ops
    assert callable(ops.score_rows_alts)
