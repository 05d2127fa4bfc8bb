"""Token-selection kernels (csrc/select.h, decode.hip, the greedy / embedding kernels of norm.hip) at the smallest shapes at
which their per-thread, per-wave and cross-wave paths differ: V = 300 (most of a 1024-thread workgroup owns no element),
V = 2500 (threads own 2 or 3 elements) and the model's V = 30522 (docs/LAB_refactor_decode.md).

References are torch on the CPU (argmax / topk / logsumexp / sigmoid) and the oracle's sampler.  Integer results and the greedy
top-2 margin (one fp32 subtraction of the same two values on both sides) are compared for equality; log-probs to fp32 summation
order (1e-5); the sampled margin to SAMPLE_MARGIN_TOL, which allows for logf of the device and of numpy differing by an ulp in
the Gumbel noise (see tests/test_hip_sample.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VS = [300, 2500, 30522]
EOS, PAD = 102, 0


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vitcap_amd import ops as o
    return o


def _ld(V):
    return (V + 63) // 64 * 64


def _init(ops, B, max_len):
    st = ops.greedy_init(B, max_len)
    st['raw_last'] = torch.full((B,), -1, dtype=torch.int64, device='cuda')
    return st


def _top2_places(V):
    """(column of the largest, column of the runner-up): owned by one thread, by two lanes of one wave, by two waves, and the
    largest in the last column.  Column c belongs to thread c % 1024, wave (c % 1024) / 64."""
    return [(5, 1029) if V > 1029 else (5, 6), (6, 5), (5, 700) if V > 700 else (5, 200), (V - 1, 5)]


@pytest.mark.parametrize('V', VS)
def test_greedy_step_places_margin_and_last_step(ops, V):
    """ids == torch.argmax (lowest index on a tie), margin == top1 - top2 exactly (0 on the tie), raw_last and the forced [SEP]
    of the last step, log-prob as test_greedy_step_bookkeeping; row 1 finishes at step 1 and stays padded."""
    B, max_len, ld = 4, 4, _ld(V)
    g = torch.Generator().manual_seed(300 + V)
    st = _init(ops, B, max_len)
    places = _top2_places(V)
    unf = torch.ones(B, dtype=torch.long)
    ids_ref = torch.zeros(B, max_len, dtype=torch.long)
    ids_ref[:, 0] = 101
    lps, unfs = [], []
    for t in range(1, max_len):
        logits = torch.randn(B, ld, generator=g)
        logits[:, V:] = 1e9                                        # padding columns must be ignored
        for b in range(B):
            hi, lo = places[(b + t) % 4]
            logits[b, hi], logits[b, lo] = 50.0 + 0.37 * b, 49.5 - 0.11 * t
        if t == 1:
            logits[1, EOS] = 60.0                                  # row 1 finishes here
        if t == 2:
            logits[2, 7] = logits[2, 200] = 55.0                   # exact tie: column 7, margin 0
        ops.greedy_step(logits.cuda(), st, t, V=V)
        row = logits[:, :V]
        top2 = torch.topk(row, 2).values
        nxt = row.argmax(-1)
        live = unf.bool()
        assert torch.equal(st['margin'][:, t].cpu()[live], (top2[:, 0] - top2[:, 1])[live]), t
        if t == 2:
            assert int(nxt[2]) == 7 and float(st['margin'][2, 2]) == 0.0
        lps.append(torch.log_softmax(row, -1).gather(1, nxt[:, None])[:, 0])
        unfs.append(unf.clone())
        add = nxt * unf
        ids_ref[:, t] = add
        last_add = add
        unf = unf * (add != EOS).long()
    assert torch.equal(st['raw_last'].cpu(), last_add)               # the chosen token, PAD for the finished row
    ids_ref[:, -1].masked_fill_(unf.bool(), EOS)
    assert torch.equal(st['ids'].cpu(), ids_ref)
    assert ids_ref[1].tolist() == [101, EOS, PAD, PAD] and int(unf.sum()) == B - 1
    assert torch.equal(st['unf'].cpu().long(), unf)
    u = torch.stack(unfs, 1).float()
    lp_ref = (torch.stack(lps, 1) * u).sum(1) / u.sum(1)
    err = (st['logprob'].cpu() - lp_ref).abs()
    print('MEASURED greedy logprob V=%d: max err %.3e' % (V, float(err.max())))
    assert bool((err <= 1e-5 + 1e-5 * lp_ref.abs()).all())


# |kernel margin - oracle margin|: the margin is the difference of two scores x + g, g = -log(-log(u)); logf of the device and of
# numpy differ by an ulp, which moves g (|g| < 17) by about an ulp of g and the rounded score by at most one ulp of the score.
# Measured on the build before the refactor, largest difference over the comparable row-steps of the 12 cases below: 1.907e-06
# (two ulp of a score in [8, 16)); the bound is 4 x that.
SAMPLE_MARGIN_TOL = 4 * 1.907e-06
SAMPLE_SEED = 41       # the oracle alone decides >= 3 of the 4 rows in all 12 cases (checked on the CPU)


def _sample_case(V, temperature, top_k, top_p):
    """Inputs and the oracle's results for B = 4 rows x 3 steps: (logits per step, tok, lp, margin, ok per step)."""
    from oracle import vitcap_oracle as O
    B, ld, seed = 4, _ld(V), SAMPLE_SEED
    g = torch.Generator().manual_seed(1000 + V)
    samp = O.make_sampler(temperature, top_k, top_p, seed=seed)
    # a row-step whose nucleus boundary moves when top_p moves by 1e-5 is undecidable at fp32 (tests/test_hip_sample.py)
    near = [O.make_sampler(temperature, top_k, top_p + d, seed=seed) for d in (-1e-5, 1e-5)] if top_p < 1 else []
    steps = []
    for t in range(1, 4):
        logits = torch.randn(B, ld, generator=g) * 4.0
        logits[:, V:] = 1e9                                        # padding columns must never be drawn
        if t == 2:
            logits[1, EOS] = 60.0                                  # forces [SEP] for row 1
        x = logits[:, :V].contiguous()
        tok, lp, margin = samp(x, t)
        ok = margin > 1e-4
        for ns in near:
            tok_n, lp_n, _ = ns(x, t)
            ok &= (tok_n == tok) & (lp_n == lp)
        steps.append((logits, tok, lp, margin, ok))
    return seed, steps


SAMPLE_PARAMS = [(1.0, 0, 1.0), (0.7, 40, 1.0), (1.0, 0, 0.9), (1.3, 200, 0.6)]


@pytest.mark.parametrize('temperature,top_k,top_p', SAMPLE_PARAMS)
@pytest.mark.parametrize('V', VS)
def test_sample_step_small_vocabularies(ops, V, temperature, top_k, top_p):
    """Tokens, log-probs and the kernel's own top-2 margin of (filtered logit + noise) against the oracle's sampler, on the rows
    the oracle itself can decide (margin > 1e-4, nucleus boundary stable under top_p +- 1e-5): at least B - 1 of them."""
    B, max_len = 4, 4
    seed, steps = _sample_case(V, temperature, top_k, top_p)
    st = _init(ops, B, max_len)
    unf = torch.ones(B, dtype=torch.long)
    ok = torch.ones(B, dtype=torch.bool)
    ids_ref = torch.zeros(B, max_len, dtype=torch.long)
    ids_ref[:, 0] = 101
    lps, unfs, worst = [], [], 0.0
    for t, (logits, tok, lp, margin, ok_t) in enumerate(steps, 1):
        ops.sample_step(logits.cuda(), st, t, temperature, top_k, top_p, seed=seed, V=V)
        ok &= ok_t | (unf == 0)
        cmp = ok & unf.bool()
        got_m = st['margin'][:, t].cpu()
        fin = torch.isfinite(margin)                                 # one survivor: both sides say +inf
        assert torch.equal(torch.isfinite(got_m)[cmp], fin[cmp]), t
        d = (got_m - margin).abs()[cmp & fin]
        worst = max(worst, float(d.max()) if d.numel() else 0.0)
        lps.append(lp)
        unfs.append(unf.clone())
        add = tok * unf
        ids_ref[:, t] = add
        last_add = add
        unf = unf * (add != EOS).long()
    ids_ref[:, -1].masked_fill_(unf.bool(), EOS)
    u = torch.stack(unfs, 1).float()
    lp_ref = (torch.stack(lps, 1) * u).sum(1) / u.sum(1)
    got = st['ids'].cpu()
    print('MEASURED sample margin V=%d T=%g k=%d p=%g: max |kernel - oracle| %.3e over %d comparable rows'
          % (V, temperature, top_k, top_p, worst, int(ok.sum())))
    assert int(ok.sum()) >= B - 1
    assert torch.equal(got[ok], ids_ref[ok]), (got, ids_ref)
    assert ids_ref[1, 2] == EOS and ids_ref[1, 3] == PAD
    assert torch.equal(st['raw_last'].cpu()[ok], last_add[ok])
    np.testing.assert_allclose(st['logprob'].cpu().numpy()[ok.numpy()], lp_ref.numpy()[ok.numpy()], atol=2e-5)
    assert worst <= SAMPLE_MARGIN_TOL


def _rowstat(logits):
    """The vocabulary GEMM's row statistics in the documented layout, [rows][pieces][4] = {max, its column (int bits, lowest on
    ties), sum exp(x - max), -} per 32-column piece, built with torch from logits [rows][pieces * 32]."""
    rows, ld = logits.shape
    x = logits.view(rows, ld // 32, 32)
    m, _ = x.max(-1)
    first = (x == m[..., None]).float().argmax(-1)                  # argmax of a 0/1 tensor: the first 1
    col = (first + torch.arange(ld // 32) * 32).to(torch.int32)
    rs = torch.zeros(rows, ld // 32, 4)
    rs[..., 0] = m
    rs[..., 1] = col.view(torch.float32)
    rs[..., 2] = torch.exp(x - m[..., None]).sum(-1)
    return rs


@pytest.mark.parametrize('k', [1, 4, 16])
@pytest.mark.parametrize('V', [300, 2500])
def test_row_topk_small_vocabularies(ops, V, k):
    """vitcap_row_topk_lse and vitcap_row_topk_pieces on 37 rows: values and columns == torch.topk (a tie across two pieces
    resolves to the lower column), logsumexp to 1e-5.  The pieces form needs pieces >= k: at V = 300 (10 pieces) k = 16 is
    refused, which is asserted instead."""
    from vitcap_amd._lib import VitcapError
    rows, ld = 37, _ld(V)
    g = torch.Generator().manual_seed(7 * V + k)
    logits = torch.randn(rows, ld, generator=g)
    logits[:, V:] = -1e30                                            # as the GEMM's padded bias leaves them
    logits[3, 40] = logits[3, 100] = 9.0                             # pieces 1 and 3
    logits[5, V - 1] = 8.0                                           # the last column
    ld_d = logits.cuda()
    want_v, want_i = torch.topk(logits[:, :V], k, dim=1)
    want_lse = torch.logsumexp(logits[:, :V].double(), 1)
    untied = (want_v[:, :-1] != want_v[:, 1:]).all(1)
    assert int(untied.sum()) >= rows - 2
    results = [('lse', ops.row_topk(ld_d, V, k))]
    rs = _rowstat(logits).cuda()
    if rs.shape[1] >= k:
        results.append(('pieces', ops.row_topk(ld_d, V, k, rowstat=rs)))
    else:
        with pytest.raises(VitcapError, match='row_topk_pieces'):
            ops.row_topk(ld_d, V, k, rowstat=rs)
    for name, (v, i, lse) in results:
        assert torch.equal(v.cpu(), want_v), name
        assert torch.equal(i.cpu().long()[untied], want_i[untied]), name
        assert i[3, 0].item() == 40 and (k == 1 or i[3, 1].item() == 100), name
        assert i[5, 0].item() == V - 1, name
        err = (lse.cpu().double() - want_lse).abs()
        print('MEASURED row_topk %s V=%d k=%d: max lse err %.3e' % (name, V, k, float(err.max())))
        assert float(err.max()) <= 1e-5, name


@pytest.mark.parametrize('k', [1, 50, 64])
@pytest.mark.parametrize('V', [300, 2500])
def test_sigmoid_topk_small_vocabularies(ops, V, k):
    B, ld = 4, _ld(V)
    g = torch.Generator().manual_seed(11 * V + k)
    logits = torch.randn(B, ld, generator=g) * 2
    logits[:, V:] = 100.0
    logits[1, 7] = logits[1, 200] = 9.0                              # tie at the top: column 7 first
    ids, prob, ln = ops.sigmoid_topk(logits.cuda(), k=k, V=V)
    p, i = torch.sort(torch.sigmoid(logits[:, :V]), dim=1, descending=True, stable=True)   # topk with the lowest index first
    p, i = p[:, :k], i[:, :k]
    assert torch.equal(ids.cpu(), i)
    assert ids[1, 0].item() == 7 and (k == 1 or ids[1, 1].item() == 200)
    err = (prob.cpu() - p).abs()
    assert bool((err <= 1e-6 + 1e-6 * p).all()), float(err.max())
    assert torch.equal(ln.cpu(), (p >= 0.2).sum(1))


def test_embed_rows_equals_embed_step(ops):
    """The teacher-forced embedding rows (vitcap_embed_rows) and the decode step's two rows (vitcap_embed_step) are the same
    (word + pos) + type -> LayerNorm: bit-identical on the rows they share, the [MASK] row included."""
    from vitcap_amd._lib import lib, check
    B, max_len, t = 5, 20, 7
    g = torch.Generator().manual_seed(31)
    word = (torch.randn(30522, 768, generator=g) * 0.05).to(torch.bfloat16).cuda()
    pos = (torch.randn(512, 768, generator=g) * 0.05).to(torch.bfloat16).cuda()
    typ = (torch.randn(2, 768, generator=g) * 0.05).to(torch.bfloat16).cuda()
    gam = (1 + torch.randn(768, generator=g) * 0.1).cuda()
    bet = (torch.randn(768, generator=g) * 0.1).cuda()
    ids = torch.randint(0, 30522, (B, max_len), generator=g)
    ids[:, t] = 103                                                  # what embed_step puts at position t
    ids = ids.cuda()
    want_f, want_b = ops.embed_step(ids, t, word, pos, typ, gam, bet)
    rows = B * max_len
    xf = torch.empty(rows, 768, device='cuda')
    xb = torch.empty(rows, 768, device='cuda', dtype=torch.bfloat16)
    p = lambda x: C.c_void_p(x.data_ptr())
    check(lib.vitcap_embed_rows(p(ids), max_len, p(word), p(pos), p(typ), p(gam), p(bet), 1e-12, None, p(xf), p(xb), rows, 0,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'embed_rows')
    got_f = xf.view(B, max_len, 768)[:, t - 1:t + 1].reshape(2 * B, 768)
    got_b = xb.view(B, max_len, 768)[:, t - 1:t + 1].reshape(2 * B, 768)
    assert torch.equal(got_f, want_f) and torch.equal(got_b, want_b)
