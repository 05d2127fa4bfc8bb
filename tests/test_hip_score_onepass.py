"""One-pass scoring of given captions: vitcap_attn_text_grid, vitcap_score_rows, vitcap_engine_score_workspace_bytes /
vitcap_engine_score_text / vitcap_engine_score (through vitcap_amd/model.py's score(one_pass=True) / score_encoded and directly).

Bounds.  Attention: |err| <= 2e-3 + 2^-7 |want| against the rounding emulation -- the project's bound for a decode-attention kernel
(tests/test_hip_ops.py).  2e-5 on log-probs computed from the same fp32 logits (tests/test_hip_forced.py).  1e-2 on a sequence
log-prob and 4e-2 per token against the reference / the fp32 oracle and between the one-pass and the stepwise path: the bounds
tests/test_hip_forced.py uses against the reference, which each path meets on its own.  Measured figures are printed as MEASURED
lines and recorded in docs/LAB_onepass_scoring.md."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GREEDY_MARGIN_FLOOR

pytestmark = pytest.mark.gpu

EOS, PAD, BOS = 102, 0, 101
V, VP, LMAX, SV = 30522, 30592, 20, 578
LP_TOL = 2e-5
SEQ_TOL = 1e-2
TOK_TOL = 4e-2


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


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


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _bf(x):
    return x.to(torch.bfloat16)


def _close(got, want, what):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    err = (got - want).abs()
    bad = err > 2e-3 + 2 ** -7 * want.abs()
    assert not bad.any(), '%s: %d/%d elements off, max err %.3e, first bad idx %s' % (
        what, int(bad.sum()), bad.numel(), float(err.max()), bad.nonzero()[:4].tolist())
    return float(err.max())


# ------------------------------------------------------------------------------------------------ 1
def _grid_mask(L):
    """(R, R) bool: text key k visible to grid row r (token row r: tokens <= r; probe j: tokens 0..j and itself)."""
    R = 2 * L - 1
    m = torch.zeros(R, R, dtype=torch.bool)
    for r in range(R):
        lim = r if r < L else r - L
        m[r, :lim + 1] = True
        if r >= L:
            m[r, r] = True
    return m


def _grid_reference(vis, text, n_img, K, L):
    """The rounding emulation per caption: keys [visual | the caption's grid rows] under the mask, softmax_pv_rounded."""
    from oracle import vitcap_oracle as O
    R = 2 * L - 1
    NC = n_img * K
    visr = vis.repeat_interleave(K, 0)                                            # (NC, 578, 2304)
    Kk = torch.cat([visr[..., 768:1536], text[..., 768:1536]], 1).float().view(NC, SV + R, 12, 64).transpose(1, 2)
    Vv = torch.cat([visr[..., 1536:], text[..., 1536:]], 1).float().view(NC, SV + R, 12, 64).transpose(1, 2)
    q = text[..., :768].float().view(NC, R, 12, 64).transpose(1, 2)
    s = q @ Kk.transpose(-1, -2)                                                  # (NC, 12, R, 578 + R)
    s[..., SV:].masked_fill_(~_grid_mask(L), float('-inf'))
    return O.softmax_pv_rounded(s, Vv, O._R(True)).transpose(1, 2).reshape(NC, R, 768)


@pytest.mark.parametrize('n_img,K,L', [(2, 1, 20), (2, 3, 20), (2, 3, 8), (2, 2, 40), (2, 2, 2), (2, 9, 20), (1, 32, 20)])
def test_attn_text_grid_vs_rounding_emulation(ops, n_img, K, L):
    """vitcap_attn_text_grid on random bf16 inputs against the oracle's rounding emulation of the decode softmax (sum from the
    unrounded P): 39 rows = a ragged third query tile, 15 rows = less than one tile, 79 rows = text keys past 64, 3 rows = one
    token and one probe, 9 and 32 captions = more than one group of 8 and the cap.  Token row L-1 (attended by nobody, feeding
    nothing) is excluded, as the contract allows; a canary 64 rows behind `out` stays intact."""
    R = 2 * L - 1
    NC = n_img * K
    vis = _bf(_rand((n_img, SV, 2304), 140 + K, 2.0))
    text = _bf(_rand((NC, R, 2304), 141 + L, 2.0))
    buf = torch.full((NC * R + 64, 768), 7.0, dtype=torch.bfloat16, device='cuda')
    got = ops.attn_text_grid(text.reshape(NC * R, 2304).cuda().contiguous(), vis.reshape(n_img * SV, 2304).cuda().contiguous(), n_img, K,
                             SV, L, out=buf)
    torch.cuda.synchronize()
    assert bool((buf[NC * R:] == 7.0).all()), 'canary behind out overwritten'
    want = _grid_reference(vis, text, n_img, K, L)
    keep = [r for r in range(R) if r != L - 1]
    worst = _close(got[:NC * R].view(NC, R, 768)[:, keep], want[:, keep], 'text-grid attention K=%d L=%d' % (K, L))
    print('MEASURED attn_text_grid n_img=%d K=%d L=%d: max |err| %.3e' % (n_img, K, L, worst))


def test_attn_text_grid_refusals(ops):
    """S_vis = 577, max_len = 41 and caps_per_image = 33 are refused by name with `out` untouched."""
    from vitcap_amd._lib import lib
    a = torch.zeros((4096, 2304), dtype=torch.bfloat16, device='cuda')
    vt = torch.zeros((1, 12, 64, 608), dtype=torch.bfloat16, device='cuda')
    out = torch.full((4096, 768), 7.0, dtype=torch.bfloat16, device='cuda')
    for K, Sv, L, name in ((1, 577, 20, b'S_vis'), (1, 578, 41, b'max_len'), (33, 578, 20, b'caps_per_image')):
        assert lib.vitcap_attn_text_grid(p(a), p(a), p(vt), p(out), 1, K, Sv, L, 0.125, S()) == -1
        assert b'attn_text_grid' in lib.vitcap_last_error() and name in lib.vitcap_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize('L', [20, 8])
def test_attn_text_grid_vs_training_form(ops, L):
    """The same kernel against independent device code: the `mask_from` form of the dense training attention on [578 visual | R
    text] rows per caption (the image's visual rows replicated per caption).  That form sums its rows through the matrix pipe
    (from the rounded P), so this is closeness within the same bound, not bit identity."""
    n_img, K = 2, 3
    R = 2 * L - 1
    NC = n_img * K
    vis = _bf(_rand((n_img, SV, 2304), 150, 2.0))
    text = _bf(_rand((NC, R, 2304), 151 + L, 2.0))
    got = ops.attn_text_grid(text.reshape(NC * R, 2304).cuda().contiguous(), vis.reshape(n_img * SV, 2304).cuda().contiguous(), n_img, K,
                             SV, L).view(NC, R, 768)
    joint = torch.cat([vis.repeat_interleave(K, 0), text], 1).reshape(NC * (SV + R), 2304).cuda().contiguous()
    want, _ = ops.attn_dense_train(joint, NC, SV + R, causal_from=SV, mask_from=SV + L, q_range=(512, SV + R))
    torch.cuda.synchronize()
    keep = [r for r in range(R) if r != L - 1]
    worst = _close(got[:, keep], want.view(NC, SV + R, 768)[:, SV:][:, keep], 'text-grid attention vs training form L=%d' % L)
    print('MEASURED attn_text_grid vs vitcap_attn_dense_fwd_train_rows L=%d: max |d| %.3e' % (L, worst))


# ------------------------------------------------------------------------------------------------ 3
def _six_captions(g, L=LMAX, eos2=1999):
    """0 runs to the end with the rule's [SEP]; 1 an explicit token in the last column; 2 ends at position 1; 3 ends mid-way with
    PAD behind it; 4 ends on the second EOS id; 5 as 0 with last_tok given."""
    c = torch.randint(2000, 30000, (6, L), generator=g)
    c[:, 0] = BOS
    c[0, -1] = EOS
    c[2, 1] = EOS
    c[2, 2:] = PAD
    c[3, 7] = EOS
    c[3, 8:] = PAD
    c[4, 5] = eos2
    c[4, 6:] = PAD
    c[5, -1] = EOS
    last = torch.full((6,), -1, dtype=torch.int64)
    last[5] = 4242
    return c, last


def test_score_rows_vs_torch_rule(ops):
    """vitcap_score_rows on synthetic logits, six caption kinds: token_logprobs and logprob within 2e-5 of float64 log_softmax,
    exact zeros at column 0 and behind the end, ids / last_tok as specified, the argmax where last_tok is absent, and two row
    chunks giving the bits of one call.  The scored tokens are likely ones (+9 on their logit), so that the sums stay below
    128 and 2e-5 is a bound on the arithmetic (docs/LAB_forced_decoding.md 2)."""
    L, eos2 = LMAX, 1999
    g = torch.Generator().manual_seed(77)
    caps, last = _six_captions(g, L, eos2)
    rows = 6 * (L - 1)
    logits = torch.randn(rows, VP, generator=g) * 2.0
    logits[:, V:] = 1e9                                               # padding columns must be ignored
    for b in range(6):
        for t in range(1, L):
            tok = int(caps[b, t])
            if tok not in (EOS, PAD, eos2):
                logits[b * (L - 1) + t - 1, tok] += 9.0
    logits[5 * (L - 1) + L - 2, 4242] += 9.0
    lsm = torch.log_softmax(logits[:, :V].double(), -1).view(6, L - 1, V)
    amax = logits[:, :V].view(6, L - 1, V).argmax(-1)
    # the rule, restated
    w_tlp = torch.zeros(6, L, dtype=torch.float64)
    w_ids = torch.zeros(6, L, dtype=torch.int64)
    w_last = torch.zeros(6, dtype=torch.int64)
    w_ids[:, 0] = BOS
    for b in range(6):
        ended = False
        for t in range(1, L):
            if ended:
                w_ids[b, t] = PAD
                if t == L - 1:
                    w_last[b] = PAD
                continue
            f = int(caps[b, t])
            if t == L - 1 and f == EOS:
                f = int(last[b]) if last[b] >= 0 else int(amax[b, t - 1])
            w_tlp[b, t] = lsm[b, t - 1, f]
            w_ids[b, t] = f
            if t == L - 1:
                w_last[b] = f
                if f not in (EOS, eos2):
                    w_ids[b, t] = EOS
            ended = f in (EOS, eos2)
    n = (w_tlp != 0).sum(1).double()
    w_lp = w_tlp.sum(1) / n
    ld, cd, lastd = logits.cuda(), caps.cuda(), last.cuda()
    one = ops.score_rows(ld, cd, last_tok=lastd, eos_extra=[eos2])
    cut = 2 * (L - 1) + 5                                             # inside caption 2
    two = ops.score_rows(ld[:cut].contiguous(), cd, last_tok=lastd, eos_extra=[eos2])
    two = ops.score_rows(ld[cut:].contiguous(), cd, st=two, rows0=cut, last_tok=lastd, eos_extra=[eos2])
    torch.cuda.synchronize()
    for k in one:
        assert torch.equal(one[k], two[k]), 'two row chunks differ from one call in %s' % k
    tlp, ids = one['token_logprobs'].cpu(), one['ids'].cpu()
    assert torch.equal(ids, w_ids) and torch.equal(one['last_tok'].cpu(), w_last)
    assert int(w_last[0]) == int(amax[0, L - 2]) and int(w_last[5]) == 4242 and int(w_last[1]) == int(caps[1, -1])
    assert ids[0, -1] == EOS and ids[1, -1] == EOS and ids[5, -1] == EOS
    assert bool((tlp[:, 0] == 0).all()) and bool((tlp[w_tlp == 0] == 0).all())
    assert one['cnt'].cpu().tolist() == [19, 19, 1, 7, 5, 19]
    e_tok = float((tlp.double() - w_tlp).abs().max())
    e_lp = float((one['logprob'].cpu().double() - w_lp).abs().max())
    e_sum = float((one['sum_lp'].cpu().double() - w_tlp.sum(1)).abs().max())
    print('MEASURED score_rows: max |token_lp - float64| %.3e, |logprob| %.3e, |sum_lp| %.3e' % (e_tok, e_lp, e_sum))
    assert e_tok <= LP_TOL and e_lp <= LP_TOL and e_sum <= LP_TOL
    # last_tok absent altogether: captions 0 and 5 both take their row's argmax
    none = ops.score_rows(ld, cd, eos_extra=[eos2])
    assert int(none['last_tok'][5]) == int(amax[5, L - 2]) and int(none['last_tok'][0]) == int(amax[0, L - 2])


# ------------------------------------------------------------------------------------------------ engine helpers
def _greedy_opts(m, **over):
    return m.gen_options(num_beams=1, do_sample=False, num_return_sequences=1, num_keep_best=1, **over)


def _raw_score(m, img, caps, K, o, last_tok=None, staged=False, sws_bytes=None, sentinel=None):
    """vitcap_engine_score (img given, whole call) or vitcap_engine_score_text (staged: the slot-0 workspace holds the prefill)
    called directly -> (rc, logprob, token_logprobs, ids, last_tok)."""
    from vitcap_amd._lib import lib
    dev = m._packed[2]
    B = caps.shape[0] // K
    ws, need = m._workspace(B, dev, 0, o)
    sneed = lib.vitcap_engine_score_workspace_bytes(B, K, C.byref(o))
    sws = torch.empty(max(sneed, 256), dtype=torch.uint8, device=dev)
    rows, L = caps.shape
    fill = (lambda *s, **k: torch.full(*s, fill_value=sentinel, **k)) if sentinel is not None else torch.empty
    lp = fill((rows,), dtype=torch.float32, device=dev)
    tlp = fill((rows, L), dtype=torch.float32, device=dev)
    ids = fill((rows, 1, L), dtype=torch.int64, device=dev)
    last = fill((rows,), dtype=torch.int64, device=dev)
    capd = caps.to(dev).contiguous()
    ltd = None if last_tok is None else last_tok.to(dev).contiguous()
    tail = (K, p(capd), p(ltd), p(sws), sneed if sws_bytes is None else sws_bytes, p(lp), p(tlp), p(ids), p(last), S())
    if staged:
        rc = lib.vitcap_engine_score_text(m._engine, B, C.byref(o), p(ws), need, *tail)
    else:
        rc = lib.vitcap_engine_score(m._engine, p(img), int(img.dtype == torch.bfloat16), B, C.byref(o), p(ws), need, *tail)
    torch.cuda.synchronize()
    return rc, lp, tlp, ids, last


# ------------------------------------------------------------------------------------------------ 4
def test_reference_goldens_one_pass_without_a_floor(model, golden):
    """test_reference_goldens_scored_without_a_floor with one_pass=True: the reference's own ids (16 + 16 + 4 images), the returned
    ids equal the given ones and the sequence log-prob of EVERY image is within 1e-2 of the reference's."""
    from vitcap_amd import weights as W
    vec, _ = golden
    pop = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_population.npz')))
    sel = _images(16, int(vec['sel_image_seed'][0]))[torch.from_numpy(vec['sel_index'])]
    cases = [('pop_noise', torch.from_numpy(W.gen_image_batch(16, int(pop['pop_noise_seed'][0]))), pop['pop_noise_ids'], pop['pop_noise_logprobs']),
             ('pop_struct', torch.from_numpy(W.gen_structured_images(16, int(pop['pop_struct_seed'][0]))), pop['pop_struct_ids'], pop['pop_struct_logprobs']),
             ('greedy_sel', sel, vec['greedy_sel_ids'], vec['greedy_sel_logprobs'])]
    worst = {}
    for name, img, ref_ids, ref_lp in cases:
        want = torch.from_numpy(ref_ids[:, 0])
        lp, tlp, ids = model.score(img.cuda(), want, return_ids=True, one_pass=True)
        assert torch.equal(ids[:, 0].cpu(), want), name
        dev = np.abs(lp.cpu().numpy() - ref_lp[:, 0])
        worst[name] = float(dev.max())
        print('MEASURED one pass %s: max |sequence log-prob - reference| %.3e (image %d), mean %.3e over %d images'
              % (name, dev.max(), int(dev.argmax()), dev.mean(), len(dev)))
    for name, w in worst.items():
        assert w <= SEQ_TOL, (name, w)


# ------------------------------------------------------------------------------------------------ 5
def test_one_pass_token_logprobs_vs_fp32_oracle(model, sd_t):
    """test_token_logprobs_vs_fp32_oracle with one_pass=True: B = 2, the oracle's fp32 greedy captions, last_tok from the oracle;
    per token within 4e-2 of log_softmax of the oracle's own logits rows, per sequence within 1e-2."""
    from oracle import vitcap_oracle as O
    img = _images(2, 1234)
    with torch.no_grad():
        ids_o, lp_o, tr = O.greedy_incremental(sd_t, img, return_trace=True)
    lp_tok = torch.zeros(2, LMAX, dtype=torch.float64)
    tok = ids_o[:, 0].clone()
    for t, stp in enumerate(tr['steps'], 1):
        if t == LMAX - 1:
            tok[:, t] = stp['logits_row'].argmax(-1)
        lp_tok[:, t] = torch.log_softmax(stp['logits_row'].double(), -1).gather(1, tok[:, t:t + 1])[:, 0]
    assert not bool((ids_o[:, 0, 1:-1] == EOS).any()), 'the recipe\'s captions run to the last position'
    lp, tlp, ids = model.score(img.cuda(), ids_o[:, 0], return_ids=True, last_tok=tok[:, -1], one_pass=True)
    assert torch.equal(ids.cpu(), ids_o)
    err = (tlp.cpu().double() - lp_tok)[:, 1:]
    print('MEASURED one pass token_logprobs vs fp32 oracle: max %.3e, rms %.3e over %d tokens' %
          (float(err.abs().max()), float(err.pow(2).mean().sqrt()), err.numel()))
    assert float(err.abs().max()) <= TOK_TOL
    assert float((lp.cpu() - lp_o[:, 0]).abs().max()) <= SEQ_TOL


# ------------------------------------------------------------------------------------------------ 6
def _variants(c, K):
    """K captions per image: its own, then its own with one word changed (positions 3, 5, ..., 17, 1, 3, ...; another word each)."""
    caps = c.repeat_interleave(K, 0).clone()
    for i in range(c.shape[0]):
        for j in range(1, K):
            caps[K * i + j, 1 + (2 * j) % 18] = 2023 + 40 * i + j
    return caps


@pytest.mark.parametrize('K', [1, 3])
def test_one_pass_vs_stepwise(model, K):
    """4 images, generate()'s own captions (K = 3: each image's own plus two with one word changed): same ids, sequence log-prob
    within 1e-2 and token log-probs within 4e-2 of the stepwise score() -- the bounds each path meets against the reference."""
    img = _images(4, 56).cuda()
    ids0, _ = model.generate(img)
    caps = _variants(ids0[:, 0].cpu(), K)
    lp_s, tlp_s, ids_s = model.score(img, caps, seqs_per_image=K, return_ids=True)
    lp_o, tlp_o, ids_o = model.score(img, caps, seqs_per_image=K, return_ids=True, one_pass=True)
    assert torch.equal(ids_o, ids_s)
    d_lp, d_tok = float((lp_o - lp_s).abs().max()), float((tlp_o - tlp_s).abs().max())
    print('MEASURED one pass vs stepwise K=%d: max |d logprob| %.3e, max |d token_lp| %.3e' % (K, d_lp, d_tok))
    assert d_lp <= SEQ_TOL and d_tok <= TOK_TOL
    assert lp_o.shape == lp_s.shape and tlp_o.shape == tlp_s.shape and ids_o.shape == ids_s.shape


def test_one_pass_vs_stepwise_early_ends_and_last_column(model):
    """A second EOS id (a word of the captions) makes captions end early: zeros and PAD behind the end, same ids and scores within
    the bounds.  Last column: with last_tok absent the one-pass argmax is the stepwise path's own choice on every row whose top-2
    margin is at least the greedy floor (at least one such row); with last_tok given both score that token."""
    img = _images(4, 56).cuda()
    ids_plain, _ = model.generate(img)
    over = {'eos_token_ids': [EOS, int(ids_plain[0, 0, 7])]}
    o = _greedy_opts(model, **over)
    ids0, lp0, last0 = model.run(img, o, want_last=True)
    ends = (ids0[:, 0] == over['eos_token_ids'][1]).any(1)
    assert bool(ends.any()), 'the second EOS id must end at least one caption early'
    caps = ids0[:, 0].cpu()
    lp_s, tlp_s, ids_s = model.score(img, caps, return_ids=True, **over)
    lp_o, tlp_o, ids_o = model.score(img, caps, return_ids=True, one_pass=True, **over)
    assert torch.equal(ids_o, ids_s) and torch.equal(ids_o, ids0)
    d_lp, d_tok = float((lp_o - lp_s).abs().max()), float((tlp_o - tlp_s).abs().max())
    print('MEASURED one pass vs stepwise, early ends: max |d logprob| %.3e, max |d token_lp| %.3e' % (d_lp, d_tok))
    assert d_lp <= SEQ_TOL and d_tok <= TOK_TOL
    behind = ids_o[:, 0] == PAD
    assert bool(behind.any()) and bool((tlp_o[behind] == 0).all()) and bool((tlp_o[:, 0] == 0).all())
    # last column, plain options: the stepwise loop's own choice and the top-2 margin of its last row
    o1 = _greedy_opts(model)
    ids1, lp1, last1 = model.run(img, o1, want_last=True)
    row = model.tap('logits_last', 4, (4, VP), opts=o1)[:, :V]
    top2 = torch.topk(row, 2).values
    margin = (top2[:, 0] - top2[:, 1]).cpu()
    open_ = ~(ids1[:, 0, 1:-1] == EOS).any(1).cpu()
    cmp = open_ & (margin >= GREEDY_MARGIN_FLOOR)
    assert bool(cmp.any()), 'no row with a last-column margin above the floor'
    rc, lp_a, tlp_a, ids_a, last_a = _raw_score(model, img, ids1[:, 0].cpu(), 1, o1)
    assert rc == 0 and torch.equal(last_a.cpu()[cmp], last1.cpu()[cmp])
    assert float((lp_a[cmp] - lp1[:, 0][cmp]).abs().max()) <= SEQ_TOL
    given = torch.full((4,), 2500, dtype=torch.int64)
    lp_gs, tlp_gs = model.score(img, ids1[:, 0].cpu(), last_tok=given)
    rc, lp_go, tlp_go, ids_go, last_go = _raw_score(model, img, ids1[:, 0].cpu(), 1, o1, last_tok=given)
    assert rc == 0 and torch.equal(last_go.cpu()[open_], given[open_]) and torch.equal(ids_go, ids1)
    d = float((tlp_go - tlp_gs).abs().max())
    print('MEASURED one pass vs stepwise, last_tok given: max |d token_lp| %.3e (%d rows compared on the argmax)' % (d, int(cmp.sum())))
    assert d <= TOK_TOL and float((lp_go - lp_gs).abs().max()) <= SEQ_TOL


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize('L', [8, 40])
def test_one_pass_other_max_lengths(model, L):
    """max_length 8 and 40 (text keys past 64) end to end, B = 2, against the stepwise score()."""
    img = _images(2, 61).cuda()
    ids0, _ = model.generate(img, max_length=L)
    caps = ids0[:, 0].cpu()
    lp_s, tlp_s, ids_s = model.score(img, caps, return_ids=True, max_length=L)
    lp_o, tlp_o, ids_o = model.score(img, caps, return_ids=True, one_pass=True, max_length=L)
    assert torch.equal(ids_o, ids_s) and tuple(tlp_o.shape) == (2, L)
    d_lp, d_tok = float((lp_o - lp_s).abs().max()), float((tlp_o - tlp_s).abs().max())
    print('MEASURED one pass vs stepwise max_length=%d: max |d logprob| %.3e, max |d token_lp| %.3e' % (L, d_lp, d_tok))
    assert d_lp <= SEQ_TOL and d_tok <= TOK_TOL


# ------------------------------------------------------------------------------------------------ 8
def test_twelve_captions_per_image(model):
    """B = 2, 12 captions per image (more than the stepwise cap of 8, two attention groups): the 24 results equal those of three
    K = 4 one-pass calls on the same images within 2e-5 -- the same arithmetic per caption, so only grouping can differ."""
    img = _images(2, 57).cuda()
    ids0, _ = model.generate(img)
    caps = _variants(ids0[:, 0].cpu(), 12)
    caps[5, 8], caps[5, 9:] = EOS, PAD                                # one early end
    lp12, tlp12, ids12 = model.score(img, caps, seqs_per_image=12, return_ids=True, one_pass=True)
    assert torch.equal(ids12[:, 0].cpu(), caps)
    c3 = caps.view(2, 3, 4, LMAX)
    exact = True
    worst = 0.0
    for j in range(3):
        lp4, tlp4, ids4 = model.score(img, c3[:, j].reshape(8, LMAX), seqs_per_image=4, return_ids=True, one_pass=True)
        sel = (torch.arange(2)[:, None] * 12 + j * 4 + torch.arange(4)[None]).reshape(-1)
        assert torch.equal(ids12[sel], ids4)
        worst = max(worst, float((lp12[sel] - lp4).abs().max()), float((tlp12[sel] - tlp4).abs().max()))
        exact = exact and torch.equal(lp12[sel], lp4) and torch.equal(tlp12[sel], tlp4)
    print('MEASURED K=12 vs 3 x K=4: max |d| %.3e, bit-identical: %s' % (worst, exact))
    assert worst <= LP_TOL
    assert float((lp12[0] - lp12[1]).abs()) > 1e-3                    # different captions score differently


# ------------------------------------------------------------------------------------------------ 9
def test_staged_form_reuses_the_prefill(model):
    """The staged encoder pass + prefill once (model.run(want_last=True) enqueues the stages one by one and then decodes),
    vitcap_engine_score_text twice with different captions: each result
    bit-identical to the whole-call vitcap_engine_score, the workspace's visual caches untouched, score_encoded() the same thin
    wrapper, and a plain generate() afterwards unchanged."""
    img = _images(3, 58).cuda()
    ids0, lp0 = model.generate(img)
    a = ids0[:, 0].cpu().clone()
    b = a.clone()
    b[:, 2] = torch.tensor([2023, 2024, 2025])
    b[1, 6], b[1, 7:] = EOS, PAD
    o = _greedy_opts(model)
    whole = [_raw_score(model, img, c, 1, o) for c in (a, b)]
    assert all(w[0] == 0 for w in whole) and not torch.equal(whole[0][1], whole[1][1])
    model.run(img, o, want_last=True)
    taps = [model.tap('dqkv%d' % l, 3, (3 * SV, 2304), dtype=torch.bfloat16, opts=o) for l in range(4)]
    assert float(taps[0][:, 768:].float().abs().max()) > 0
    for c, w in zip((b, a), (whole[1], whole[0])):
        got = _raw_score(model, None, c, 1, o, staged=True)
        assert got[0] == 0
        for x, y in zip(got[1:], w[1:]):
            assert torch.equal(x, y)
    for l in range(4):                                                # K | V columns: what the prefill wrote in every layer
        assert torch.equal(model.tap('dqkv%d' % l, 3, (3 * SV, 2304), dtype=torch.bfloat16, opts=o)[:, 768:], taps[l][:, 768:])
    # the model-level staged form: the images of the last score() call on the slot
    lp_w, tlp_w, ids_w = model.score(img, b, return_ids=True, one_pass=True)
    lp_e, tlp_e, ids_e = model.score_encoded(a, return_ids=True)
    assert torch.equal(lp_w, whole[1][1]) and torch.equal(lp_e, whole[0][1]) and torch.equal(tlp_e, whole[0][2]) and torch.equal(ids_e, whole[0][3])
    ids1, lp1 = model.generate(img)
    assert torch.equal(ids1, ids0) and torch.equal(lp1, lp0)


# ------------------------------------------------------------------------------------------------ 10
def test_engine_score_refusals_on_the_device(model):
    """Every refused option returns VITCAP_EINVAL with its name and leaves the outputs' sentinel; a score workspace one byte
    short returns VITCAP_EWORKSPACE."""
    from vitcap_amd import _lib as L
    lib = L.lib
    img = _images(1, 59).cuda()
    caps = torch.full((1, LMAX), 2000, dtype=torch.int64)
    caps[:, 0], caps[:, -1] = BOS, EOS
    model.generate(img)
    fsm = torch.zeros(8, dtype=torch.uint8, device='cuda')
    refused = ((L.gen_opts(num_beams=2), b'num_beams'),
               (L.gen_opts(use_cbs=1, cbs_states=8, fsm=fsm.data_ptr(), num_constraints=fsm.data_ptr()), b'use_cbs'),
               (L.gen_opts(tag_visible=5), b'tag_visible'),
               (L.gen_opts(sampling=L.SampleParams(1, 1.0, 0, 1.0, 0)), b'do_sample'),
               (L.gen_opts(repetition_penalty=1.3), b'repetition_penalty'))
    o = _greedy_opts(model)

    def untouched(r):
        return bool((r[1] == -7).all()) and bool((r[2] == -7).all()) and bool((r[3] == -7).all()) and bool((r[4] == -7).all())

    for staged in (False, True):
        for bad, name in refused:
            r = _raw_score(model, img, caps, 1, bad, staged=staged, sentinel=-7)
            assert r[0] == -1 and name in lib.vitcap_last_error() and untouched(r), name
        r = _raw_score(model, img, caps.repeat(33, 1), 33, o, staged=staged, sentinel=-7)
        assert r[0] == -1 and b'caps_per_image' in lib.vitcap_last_error() and untouched(r)
        need = lib.vitcap_engine_score_workspace_bytes(1, 1, C.byref(o))
        r = _raw_score(model, img, caps, 1, o, staged=staged, sws_bytes=need - 1, sentinel=-7)
        assert r[0] == -3 and untouched(r)
    ws, wneed = model._workspace(1, model._packed[2], 0, o)
    a = p(ws)
    assert lib.vitcap_engine_score(model._engine, p(img), 0, 1, C.byref(o), a, wneed, 1, None, None, a, 1 << 40, a, None, a, None, S()) == -1
    assert b'null' in lib.vitcap_last_error()
    assert lib.vitcap_engine_score_text(model._engine, 1, C.byref(o), a, wneed, 1, a, None, a, 1 << 40, None, None, a, None, S()) == -1
    r = _raw_score(model, img, caps, 1, o, sentinel=-7)               # and the accepted call writes every output
    assert r[0] == 0 and not untouched(r) and bool(torch.isfinite(r[1]).all())
