"""Token alternatives of given captions on the device: vitcap_score_rows_alts (through ops.score_rows_alts), vitcap_engine_score_req
with kind VITCAP_SCORE_ALTS (through vitcap_amd/model.py's alternatives / alternatives_encoded / caption_with_alternatives) and
the pipeline's `alternatives: k`.

Bounds.  The op against the fp64 restatement of the row rule (tests/alternatives_ref.py): alt_ids and rank exact; alt_lp within 2e-5
(the bound tests/test_hip_forced.py 1-3 use for this arithmetic); entropy within 64 * 2^-24 * (|log S| + |T| / S) per row, taken from
the restatement (30 serial + 10 tree additions on an element's path plus a few ulp of expf / logf, rounded up).  Against
vitcap_score_rows and score(one_pass=True): bit for bit.  Against the fp32 oracle: TOK_TOL = 4e-2 per token log-prob, the bound of
tests/test_hip_forced.py 7, propagated to order, rank and entropy as the tests state.  Measured figures are printed as MEASURED lines
and recorded in docs/LAB_alternatives.md."""
import json
import os

import numpy as np
import pytest
import torch

import alternatives_ref as R
from test_hip_score_onepass import _images, _variants

pytestmark = pytest.mark.gpu

EOS, PAD, BOS = 102, 0, 101
EOS2 = 1012
V_REAL, VP = 30522, 30592
LMAX = 20
TOK_TOL = 4e-2
SENT = 777
# (V, ldl, k): the real vocabulary with its padded stride; V = 1000: threads without an element; 1025 / 2048: the boundaries of the
# thread stride; V = 16 = k: every entry is an alternative
OP_CASES = ((V_REAL, VP, 1), (V_REAL, VP, 5), (V_REAL, VP, 16), (1000, 1003, 5), (1025, 1025, 5), (2048, 2048, 16), (16, 19, 16))


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


# ------------------------------------------------------------------------------------------------ inputs, shared and never modified
_INPUTS = {}


def _planted(V, ldl):
    """The eight planted rows as two captions of L = 5, every position live, cap[t] = the token the row is to be scored on."""
    key = ('planted', V, ldl)
    if key not in _INPUTS:
        logits, f = R.planted_rows(V, seed=31 + V, ld=ldl)
        ids = np.full((2, 5), BOS, np.int64)
        ids[:, 1:] = f.reshape(2, 4)
        _INPUTS[key] = (logits, ids, None)
    return _INPUTS[key]


def _ranged(V, ldl):
    """Six captions of L = 8 on random rows: 0 ends at position 2 (dead rows behind it); 1 / 2 run to the last column and hold the
    max-length rule's [SEP] there, with / without a last_tok; 3 ends on the second EOS id; 4 holds an id outside the vocabulary and an
    explicit word in the last column; 5 is plain.  The given word of every second row is a likely one (+9 on its logit)."""
    key = ('ranged', V, ldl)
    if key not in _INPUTS:
        rng = np.random.RandomState(7 + V)
        L = 8
        ids = rng.randint(1, V, (6, L)).astype(np.int64)
        ids[(ids == EOS) | (ids == EOS2)] = 1
        ids[:, 0] = BOS
        ids[0, 2], ids[0, 3:] = EOS, PAD
        ids[1, -1] = ids[2, -1] = EOS
        ids[3, 3], ids[3, 4:] = EOS2, PAD
        ids[4, 2] = V + 5
        last = np.array([-1, min(V - 1, 4242), -1, -1, -1, -1], np.int64)
        logits = np.full((6 * (L - 1), ldl), 1e9, np.float32)                # the columns behind V must be ignored
        logits[:, :V] = (rng.randn(6 * (L - 1), V) * 2.0).astype(np.float32)
        for g in range(0, 6 * (L - 1), 2):
            tok = ids[g // (L - 1), g % (L - 1) + 1]
            if 0 <= tok < V:
                logits[g, tok] += 9.0
        _INPUTS[key] = (logits, ids, last)
    return _INPUTS[key]


_REFS = {}


def _ref(kind, V, ldl, k, rows0=0, n_rows=None, with_last=True):
    key = (kind, V, ldl, k, rows0, n_rows, with_last)
    if key not in _REFS:
        logits, ids, last = (_planted if kind == 'planted' else _ranged)(V, ldl)
        n = logits.shape[0] - rows0 if n_rows is None else n_rows
        _REFS[key] = R.alternatives_ref(logits[rows0:rows0 + n], V, ids, k, rows0=rows0, last_tok=last if with_last else None,
                                        eos_extra=(EOS2,))
    return _REFS[key]


def _framed(shape, dtype, pad=256):
    """A sentinel-filled buffer with `shape` in its middle -> (whole buffer, the view)."""
    n = int(np.prod(shape))
    buf = torch.full((pad + n + pad,), SENT, dtype=dtype, device='cuda')
    return buf, buf[pad:pad + n].view(shape)


def _run_op(ops, kind, V, ldl, k, rows0=0, n_rows=None, with_last=True):
    """vitcap_score_rows_alts into sentinel-framed arrays -> (outputs on the host, canaries intact)."""
    logits, ids, last = (_planted if kind == 'planted' else _ranged)(V, ldl)
    n = logits.shape[0] - rows0 if n_rows is None else n_rows
    n_caps, L = ids.shape
    bufs, out = {}, {}
    for name, shape, dt in (('ids', (n_caps, L, k), torch.int32), ('logprobs', (n_caps, L, k), torch.float32),
                            ('rank', (n_caps, L), torch.int32), ('entropy', (n_caps, L), torch.float32)):
        bufs[name], out[name] = _framed(shape, dt)
    ld = torch.from_numpy(logits[rows0:rows0 + n]).cuda()
    assert ld.stride(0) == ldl
    lt = torch.from_numpy(last).cuda() if (last is not None and with_last) else None
    ops.score_rows_alts(ld, torch.from_numpy(ids).cuda(), k, out=out, rows0=rows0, last_tok=lt, V=V, eos_extra=[EOS2])
    torch.cuda.synchronize()
    ok = all(bool((bufs[n_][:256] == SENT).all()) and bool((bufs[n_][256 + out[n_].numel():] == SENT).all()) for n_ in bufs)
    return {n_: out[n_].cpu().numpy() for n_ in out}, ok


def _compare(got, ref, what):
    """Covered positions against the restatement, uncovered ones against the sentinel -> (max |alt_lp - f64|, max entropy error in
    units of its bound)."""
    c = ref['covered']
    assert (got['ids'][c] == ref['ids'][c]).all(), what
    assert (got['rank'][c] == ref['rank'][c]).all(), what
    assert (got['ids'][~c] == SENT).all() and (got['rank'][~c] == SENT).all(), what
    assert (got['logprobs'][~c] == SENT).all() and (got['entropy'][~c] == SENT).all(), what
    dead = c & ~ref['live']
    assert (got['logprobs'][dead] == 0).all() and (got['entropy'][dead] == 0).all() and (got['ids'][dead] == -1).all(), what
    e_lp = float(np.abs(got['logprobs'][c].astype(np.float64) - ref['lp'][c]).max())
    live = c & ref['live']
    e_ent = np.abs(got['entropy'][live].astype(np.float64) - ref['entropy'][live])
    tol = ref['ent_tol'][live]
    worst = float(np.where(tol > 0, e_ent / np.where(tol > 0, tol, 1), np.where(e_ent > 0, np.inf, 0)).max()) if live.any() else 0.0
    return e_lp, worst


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize('V,ldl,k', OP_CASES, ids=lambda v: str(v))
def test_op_against_the_restatement(ops, V, ldl, k):
    """vitcap_score_rows_alts on the planted rows and on the six caption kinds (whole range; a range that starts and ends inside
    captions; the last-column row of caption 1 without any last_tok): alt_ids and rank exact, alt_lp within 2e-5 of fp64, entropy
    within its per-row bound, the dead pattern behind a caption's end, column 0, the uncovered positions and the canaries untouched."""
    runs = (('planted', 0, None, True), ('ranged', 0, None, True), ('ranged', 9, 20, True), ('ranged', 13, 1, False))
    worst_lp = worst_ent = 0.0
    for kind, rows0, n_rows, with_last in runs:
        got, canaries = _run_op(ops, kind, V, ldl, k, rows0, n_rows, with_last)
        ref = _ref(kind, V, ldl, k, rows0, n_rows, with_last)
        what = (kind, V, k, rows0, n_rows)
        assert canaries, what
        assert not ref['covered'][:, 0].any() and int(ref['covered'].sum()) == (n_rows or ref['covered'][:, 1:].size), what
        e_lp, e_ent = _compare(got, ref, what)
        worst_lp, worst_ent = max(worst_lp, e_lp), max(worst_ent, e_ent)
    print('MEASURED score_rows_alts V=%d ldl=%d k=%d: max |alt_lp - float64| %.3e (bound 2e-5), max entropy error %.3f of its bound'
          % (V, ldl, k, worst_lp, worst_ent))
    assert worst_lp <= R.LP_TOL and worst_ent <= 1.0
    # what the planted rows are there for, on the device's own output
    got, _ = _run_op(ops, 'planted', V, ldl, k)
    rank, ent = got['rank'].reshape(-1, 5)[:, 1:].reshape(-1), got['entropy'].reshape(-1, 5)[:, 1:].reshape(-1)
    ids = got['ids'].reshape(2, 5, k)[:, 1:].reshape(8, k)
    f = _planted(V, ldl)[1][:, 1:].reshape(-1)
    assert rank[0] == 0 and ids[0, 0] == f[0] and rank[1] == V - 1 and rank[2] == 1 and rank[3] == 0 and rank[5] == V // 2
    assert rank[4] == 1 and (k < 2 or ids[4, :2].tolist() == [3, int(f[4])])          # -0.0 at index 3 comes before +0.0 behind it
    assert abs(float(ent[5]) - np.log(V)) <= 64 * 2.0 ** -24 * np.log(V) and ids[5].tolist() == list(range(k))
    assert ent[6] == 0.0 and got['logprobs'].reshape(2, 5, k)[1, 3, 0] == 0.0          # dominated: the others' expf underflow
    # the last-column rule: caption 1 scores last_tok, caption 2 (and caption 1 without last_tok) the argmax
    whole, none = _ref('ranged', V, ldl, k), _ref('ranged', V, ldl, k, 13, 1, False)
    assert whole['f'][1, 7] == min(V - 1, 4242) and whole['rank'][2, 7] == 0 and none['rank'][1, 7] == 0 and whole['rank'][4, 2] == 0
    assert whole['live'][0].tolist() == [False, True, True] + [False] * 5 and whole['live'][3].tolist() == [False] + [True] * 3 + [False] * 4


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize('V,ldl', [(V_REAL, VP), (1000, 1003)], ids=lambda v: str(v))
def test_bit_identity_with_score_rows(ops, V, ldl):
    """vitcap_score_rows on the same logits: wherever an alternative is the scored token its log-prob has token_logprobs' bits, and
    rank == 0 exactly where the first alternative is the scored token."""
    k, hits = 16, 0
    for kind in ('planted', 'ranged'):
        logits, ids, last = (_planted if kind == 'planted' else _ranged)(V, ldl)
        ld, idd = torch.from_numpy(logits).cuda(), torch.from_numpy(ids).cuda()
        lt = torch.from_numpy(last).cuda() if last is not None else None
        st = ops.score_rows(ld, idd, last_tok=lt, V=V, eos_extra=[EOS2])
        out = ops.score_rows_alts(ld, idd, k, last_tok=lt, V=V, eos_extra=[EOS2])
        torch.cuda.synchronize()
        ref = _ref(kind, V, ldl, k)
        f = torch.from_numpy(ref['f'])
        live = torch.from_numpy(ref['live'])
        a_ids, a_lp, rank = out['ids'].cpu().long(), out['logprobs'].cpu(), out['rank'].cpu()
        tlp = st['token_logprobs'].cpu()
        same = (a_ids == f[..., None]) & live[..., None]
        hits += int(same.sum())
        assert torch.equal(a_lp.view(torch.int32)[same], tlp[..., None].expand_as(a_lp).contiguous().view(torch.int32)[same]), kind
        assert torch.equal((rank == 0)[live], (a_ids[..., 0] == f)[live]), kind
        assert bool((rank[~live] == -1).all()) and bool((tlp[~live] == 0).all())
        assert bool((a_lp[..., 0][live] <= 0).all()) and float((a_lp[..., 0][live] - tlp[live]).min()) >= 0.0      # the best is the best
    assert hits >= 10, hits


# ------------------------------------------------------------------------------------------------ engine helpers
def _identities(caps, tlp, alts, what, eos_ids=(EOS,)):
    """The identities of test 2 on an engine result -> the number of alternatives that are their position's scored token."""
    caps, tlp = caps.cpu(), tlp.cpu()
    a_ids, a_lp, rank, ent = (x.cpu() for x in alts)
    L = caps.shape[1]
    live = torch.from_numpy(R.live_rows(caps.numpy(), eos_extra=eos_ids))
    f = caps.clone()
    rule = live[:, -1] & (caps[:, -1] == EOS)           # no last_tok is handed over: the row's argmax is scored there
    f[rule, -1] = a_ids[rule, -1, 0].long()
    assert bool((a_ids[~live] == -1).all()) and bool((rank[~live] == -1).all()) and bool((a_lp[~live] == 0).all()) and bool((ent[~live] == 0).all()), what
    assert bool((a_ids[live] >= 0).all()) and bool((a_ids[live] < V_REAL).all()) and bool((rank[live] >= 0).all()) and bool((ent[live] > 0).all()), what
    same = (a_ids.long() == f[..., None]) & live[..., None]
    assert torch.equal(a_lp.view(torch.int32)[same], tlp[..., None].expand_as(a_lp).contiguous().view(torch.int32)[same]), what
    assert torch.equal((rank == 0)[live], (a_ids[..., 0].long() == f)[live]), what
    assert bool((a_lp[live][:, :-1] >= a_lp[live][:, 1:]).all()), what                     # best first
    mass = float(a_lp[live].double().exp().sum(-1).max())
    assert mass <= 1 + 1e-6, (what, mass)
    assert L == tlp.shape[1]
    return int(same.sum())


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize('B,K', [(2, 1), (2, 3), (4, 32)])
def test_engine_alternatives(model, B, K):
    """alternatives() on generate()'s own captions and their variants: scores, per-token log-probs and ids are score(one_pass=True)'s
    bit for bit; the identities of test 2 hold (at 4 x 32 = 2432 probe rows in both chunks of the vocabulary GEMM); the k
    probabilities of a position sum to at most 1; alternatives_encoded gives the same bits; generate() is unchanged around the calls."""
    k = 5
    img = _images(B, 56).cuda()
    ids0, lp0 = model.generate(img)
    caps = _variants(ids0[:, 0].cpu(), K)
    lp_s, tlp_s, ids_s = model.score(img, caps, seqs_per_image=K, return_ids=True, one_pass=True)
    lp_a, tlp_a, alts = model.alternatives(img, caps, seqs_per_image=K, k=k)
    assert torch.equal(lp_a, lp_s) and torch.equal(tlp_a, tlp_s)
    assert tuple(alts.ids.shape) == (B * K, LMAX, k) and alts.ids.dtype == torch.int32 and alts.rank.dtype == torch.int32
    assert tuple(alts.entropy.shape) == (B * K, LMAX) and alts.logprobs.dtype == torch.float32
    _, _, ids_a, _ = model._score_one_pass(img, B, model.gen_options(num_beams=1, do_sample=False, num_return_sequences=1, num_keep_best=1),
                                           caps, None, K, 0, img.device, True, alts=k)
    assert torch.equal(ids_a, ids_s)
    hits = _identities(caps, tlp_a, alts, (B, K))
    assert hits > 0
    if B * K * (LMAX - 1) > 2048:                       # the second chunk starts inside caption 2048 // 19 = 107
        cut = 2048 // (LMAX - 1)
        part = lambda sl: type(alts)(*(x[sl] for x in alts))
        h0 = _identities(caps[:cut], tlp_a[:cut], part(slice(0, cut)), 'first chunk')
        h1 = _identities(caps[cut + 1:], tlp_a[cut + 1:], part(slice(cut + 1, None)), 'second chunk')
        assert h0 > 0 and h1 > 0
    lp_e, tlp_e, alts_e = model.alternatives_encoded(caps, seqs_per_image=K, k=k)
    assert torch.equal(lp_e, lp_a) and torch.equal(tlp_e, tlp_a) and all(torch.equal(x, y) for x, y in zip(alts_e, alts))
    _, _, alts16 = model.alternatives_encoded(caps, seqs_per_image=K, k=16)
    assert torch.equal(alts16.ids[..., :k], alts.ids) and torch.equal(alts16.logprobs[..., :k], alts.logprobs)
    assert torch.equal(alts16.rank, alts.rank) and torch.equal(alts16.entropy, alts.entropy)
    ids1, lp1 = model.generate(img)
    assert torch.equal(ids1, ids0) and torch.equal(lp1, lp0)
    share = float((alts.rank[alts.rank >= 0] == 0).float().mean())
    print('MEASURED engine alternatives B=%d K=%d: %d alternatives are their position\'s scored word, %.3f of the live positions at rank 0'
          % (B, K, hits, share))


@pytest.mark.parametrize('L', [8, 40])
def test_engine_alternatives_other_max_lengths(model, L):
    img = _images(1, 61).cuda()
    ids0, _ = model.generate(img, max_length=L)
    caps = ids0[:, 0].cpu()
    lp_s, tlp_s = model.score(img, caps, one_pass=True, max_length=L)
    lp_a, tlp_a, alts = model.alternatives(img, caps, k=3, max_length=L)
    assert torch.equal(lp_a, lp_s) and torch.equal(tlp_a, tlp_s) and tuple(alts.ids.shape) == (1, L, 3)
    assert _identities(caps, tlp_a, alts, L) > 0
    _, _, alts_e = model.alternatives_encoded(caps, k=3, max_length=L)
    assert all(torch.equal(x, y) for x, y in zip(alts_e, alts))


# ------------------------------------------------------------------------------------------------ 4
def test_alternatives_vs_fp32_oracle(model, sd_t):
    """B = 2: the oracle's fp32 greedy captions, last_tok from the oracle; every position against the oracle's own logits rows
    (return_trace), no position excluded: each alternative's log-prob within TOK_TOL of the oracle's for that id; the j-th alternative
    no worse in the oracle than its j-th best by more than 2 TOK_TOL; the rank between the counts of the oracle's entries clearly
    above and not clearly below the scored word; the entropy within the first-order propagation of the per-logit bound."""
    from oracle import vitcap_oracle as O
    k = 16
    img = _images(2, 1234)
    with torch.no_grad():
        ids_o, lp_o, tr = O.greedy_incremental(sd_t, img, return_trace=True)
    tok = ids_o[:, 0].clone()
    tok[:, -1] = tr['steps'][-1]['logits_row'].argmax(-1)                  # what the oracle chose there (the ids hold the forced [SEP])
    assert not bool((ids_o[:, 0, 1:-1] == EOS).any()), 'the recipe\'s captions run to the last position'
    lp, tlp, alts = model.alternatives(img.cuda(), ids_o[:, 0], k=k, last_tok=tok[:, -1])
    a_ids, a_lp, rank, ent = (x.cpu() for x in alts)
    e_lp, e_ord, e_ent, n_rank = [], [], [], 0
    for t, stp in enumerate(tr['steps'], 1):
        lsm = torch.log_softmax(stp['logits_row'].double(), -1)            # (2, V)
        for c in range(2):
            lo, f = lsm[c], int(tok[c, t])
            idx = a_ids[c, t].long()
            assert bool((idx >= 0).all())
            e_lp.append((a_lp[c, t].double() - lo[idx]).abs())
            top = torch.topk(lo, k).values
            e_ord.append(top - lo[idx])                                    # > 0: the alternative is worse in the oracle than its j-th best
            lower, upper = int((lo > lo[f] + 2 * TOK_TOL).sum()), int((lo >= lo[f] - 2 * TOK_TOL).sum())
            assert lower <= int(rank[c, t]) <= upper, (c, t, lower, int(rank[c, t]), upper)
            n_rank += int(rank[c, t]) == int((lo > lo[f]).sum())
            p = lo.exp()
            H = float(-(p * lo).sum())
            bound = 2 * TOK_TOL * float((p * (lo + H).abs()).sum())
            e_ent.append((abs(float(ent[c, t]) - H), bound))
    e_lp, e_ord = torch.stack(e_lp), torch.stack(e_ord)
    worst_ent = max(e / b for e, b in e_ent)
    print('MEASURED alternatives vs fp32 oracle: |alt_lp - lp_o| max %.3e rms %.3e over %d; order slack max %.3e (bound %.1e); '
          'rank equals the oracle\'s at %d of %d positions; |entropy - H_o| max %.3e rms %.3e, worst %.3f of its bound'
          % (float(e_lp.max()), float(e_lp.pow(2).mean().sqrt()), e_lp.numel(), float(e_ord.max()), 2 * TOK_TOL, n_rank, len(e_ent),
             max(e for e, _ in e_ent), float(np.sqrt(np.mean([e * e for e, _ in e_ent]))), worst_ent))
    assert float(e_lp.max()) <= TOK_TOL
    assert float(e_ord.max()) <= 2 * TOK_TOL
    assert worst_ent <= 1.0


# ------------------------------------------------------------------------------------------------ 5
def test_caption_with_alternatives(model):
    """ids and logprobs are generate()'s; the best alternative of the one-pass pass beats the step loop's log-prob of the chosen word
    by at most 2 TOK_TOL (each pass is within TOK_TOL of the reference); the share of chosen words at rank 0 is printed."""
    img = _images(4, 56).cuda()
    ids0, lp0, tlp0 = model.generate(img, want_token_logprobs=True)
    ids, lp, alts, tlp1 = model.caption_with_alternatives(img, k=5, want_token_logprobs=True)
    assert torch.equal(ids, ids0) and torch.equal(lp, lp0)
    ids_b, lp_b, alts_b = model.caption_with_alternatives(img, k=5)
    assert torch.equal(ids_b, ids0) and all(torch.equal(x, y) for x, y in zip(alts_b, alts))
    live = alts.rank >= 0
    assert torch.equal(live.cpu(), torch.from_numpy(R.live_rows(ids0[:, 0].cpu().numpy())))
    share = float((alts.rank[live] == 0).float().mean())
    gap = float((alts.logprobs[..., 0] - tlp0)[live].max())
    print('MEASURED caption_with_alternatives: %.3f of %d chosen words at rank 0 of the one-pass pass; max best-alternative log-prob '
          'minus the step loop\'s log-prob of the chosen word %.3e; max |one-pass - step loop| token log-prob %.3e'
          % (share, int(live.sum()), gap, float((tlp1 - tlp0)[live].abs().max())))
    assert gap <= 2 * TOK_TOL


# ------------------------------------------------------------------------------------------------ 6
class _Tok:
    def __init__(self, toks):
        self.ids_to_tokens = toks


@pytest.mark.parametrize('n_img', (2, 5))
def test_pipeline_writes_the_alternatives_tsv(model, tmp_path, monkeypatch, n_img):
    """ensure_predict with `alternatives: 3` on 2 images and on 5: the .alt.tsv rows hold, per live position of the predicted caption,
    the word, its one-pass log-prob, rank, entropy and the 3 alternatives as to_words gives them; the prediction TSV is byte-identical
    to a run without the key; every combination the alternatives are not built for is refused by name."""
    from oracle import vitcap_oracle as O
    from vitcap_amd.alternatives import to_words
    from vitcap_amd.pipeline import CaptionUniPipeline
    monkeypatch.chdir(tmp_path)
    enc = tmp_path / 'enc'
    enc.mkdir()
    toks = ['[PAD]'] + ['w%d' % i for i in range(1, 30522)]
    toks[100], toks[101], toks[102], toks[103] = '[UNK]', '[CLS]', '[SEP]', '[MASK]'
    (enc / 'vocab.txt').write_text('\n'.join(toks) + '\n')
    img = _images(n_img)
    keys = ['k%d' % i for i in range(n_img)]

    def batch():
        input_ids, am = O.test_text_inputs(n_img)
        return {'image': img.clone(), 'key': list(keys), 'input_ids': input_ids, 'attention_mask': am,
                'token_type_ids': torch.zeros(n_img, 70, dtype=torch.long)}

    def run(name, force=True, **kw):
        pl = CaptionUniPipeline(full_expid='E', init_recipe_seed=0, text_encoder_type=str(enc), tagemb='cls', force_predict=force,
                                test_batches=[batch()], model_file=str(tmp_path / (name + '.pt')), **kw)
        return pl.ensure_predict()

    plain = run('plain')
    with_alts = run('alts', alternatives=3)
    assert open(plain, 'rb').read() == open(with_alts, 'rb').read()
    assert not os.path.exists(plain[:-4] + '.alt.tsv')
    alt = with_alts[:-4] + '.alt.tsv'
    assert with_alts.endswith('.predict.tsv') and os.path.isfile(alt) and os.path.isfile(alt[:-4] + '.lineidx')
    ids, lp, alts, tlp = model.caption_with_alternatives(img.cuda(), k=3, want_token_logprobs=True, gemm_mode=1)      # the predict loop's GEMM mode
    alts_h = type(alts)(*(x.cpu() for x in alts))
    rows = [l.rstrip('\n').split('\t') for l in open(alt)]
    assert [r[0] for r in rows] == keys
    for b, (key, js) in enumerate(rows):
        recs = json.loads(js)
        words = to_words(_Tok(toks), alts_h, b)
        live = [t for t in range(1, LMAX) if int(alts_h.rank[b, t]) >= 0]
        assert len(recs) == len(live) > 0
        for rec, t in zip(recs, live):
            assert rec['word'] == toks[int(ids[b, 0, t])] and rec['rank'] == int(alts_h.rank[b, t])
            assert rec['logprob'] == float(tlp[b, t]) and rec['entropy'] == float(alts_h.entropy[b, t])
            assert rec['alternatives'] == [[w, q] for w, q in words[t]] and len(rec['alternatives']) == 3
    for kw, name in (({'num_beams': 2}, 'num_beams'), ({'use_cbs': True}, 'use_cbs'), ({'caption_prefix': 'w5 w6'}, 'caption_prefix'),
                     ({'tag_visible': 5}, 'tag_visible'), ({'attention_maps': True}, 'attention_maps')):
        with pytest.raises(NotImplementedError, match=name):
            run('refused', alternatives=3, **kw)
