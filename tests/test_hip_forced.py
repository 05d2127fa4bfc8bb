"""Forced tokens in the decode loop (caption prefixes, caption scoring), all through the C ABI.

Op level: vitcap_greedy_step_forced, vitcap_greedy_select_embed_forced and vitcap_sample_step_forced against a torch restatement of
the one rule of include/vitcap_hip.h.  Engine level: vitcap_engine_generate_forced / vitcap_engine_decode_forced (through
vitcap_amd/model.py's run / generate / score) against the plain calls, the reference's goldens, the oracle and themselves under
a replayed graph.

Bounds.  2e-5 on log-probs computed from the same fp32 logits (the bound tests/test_hip_select.py uses for the unforced kernels).
1e-2 on a sequence log-prob against the reference's fp32 run (the bound tests/test_hip_e2e.py uses for this quantity).  4e-2 per
token against the fp32 oracle: |d lp| <= |d x_f| + |d lse| <= 2 x the 2e-2 per-logit maximum test_per_step_logits_vs_reference
allows.  Measured figures are printed as MEASURED lines and recorded in docs/LAB_forced_decoding.md."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GREEDY_MARGIN_FLOOR, assert_tokens_match_reference, comparable_prefix, relevant_margins
from test_forced_cpu import forced_sampler

pytestmark = pytest.mark.gpu

EOS, PAD, BOS = 102, 0, 101
V, VP, LMAX = 30522, 30592, 20
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


def _state(ops, B, max_len):
    st = ops.greedy_init(B, max_len)
    st['raw_last'] = torch.full((B,), -1, dtype=torch.int64, device='cuda')
    st['tok_lp'] = torch.zeros((B, max_len), device='cuda')          # the caller zeroes it; the kernels write the taken positions
    return st


class Rule(object):
    """The rule of vitcap_greedy_step_forced restated with torch on the host, in float64."""

    def __init__(self, B, max_len, forced, score_forced):
        self.forced, self.sf, self.L = forced, bool(score_forced), max_len
        self.ids = torch.zeros(B, max_len, dtype=torch.long)
        self.ids[:, 0] = BOS
        self.unf = torch.ones(B, dtype=torch.long)
        self.sum_lp = torch.zeros(B, dtype=torch.float64)
        self.cnt = torch.zeros(B, dtype=torch.float64)
        self.tok_lp = torch.zeros(B, max_len, dtype=torch.float64)
        self.raw_last = None

    def step(self, t, free_tok, lsm):
        """free_tok (B,): what the step would choose; lsm (B, V) float64: the log-softmax a taken token is scored on."""
        f = self.forced[:, t]
        isf = (f >= 0) & (f < V)
        tok = torch.where(isf, f, free_tok)
        lp = lsm.gather(1, tok[:, None])[:, 0]
        live = self.unf.bool()
        counted = live & (~isf | self.sf)
        self.sum_lp += torch.where(counted, lp, torch.zeros_like(lp))
        self.cnt += counted.double()
        self.tok_lp[:, t] = torch.where(live, lp, torch.zeros_like(lp))
        add = tok * self.unf                                          # PAD = 0 for a finished sequence
        self.ids[:, t] = add
        self.unf = self.unf * (add != EOS).long()
        if t == self.L - 1:
            self.raw_last = add.clone()
            self.ids[:, t].masked_fill_(self.unf.bool(), EOS)
        return tok

    @property
    def logprob(self):
        return torch.where(self.cnt > 0, self.sum_lp / self.cnt.clamp(min=1), torch.zeros_like(self.sum_lp))

    def check(self, st, what):
        assert torch.equal(st['ids'].cpu(), self.ids), what
        assert torch.equal(st['unf'].cpu().long(), self.unf), what
        assert torch.equal(st['cnt'].cpu().double(), self.cnt), what
        assert torch.equal(st['raw_last'].cpu(), self.raw_last), what
        worst = 0.0
        for name, got, want in (('sum_lp', st['sum_lp'], self.sum_lp), ('logprob', st['logprob'], self.logprob),
                                ('token_logprobs', st['tok_lp'], self.tok_lp)):
            err = float((got.cpu().double() - want).abs().max())
            worst = max(worst, err)
            assert err <= LP_TOL, (what, name, err)
        return worst


def _six_rows(g, max_len=LMAX):
    """forced ids of the six row kinds: 0 free; 1 fully forced, [SEP] forced at the last position; 2 a prefix of 3 then free;
    3 a forced [SEP] at step 4 with junk forced behind it; 4 forced to the last position, never finishing; 5 forced with the
    argmax itself (filled in per step by the caller, from row 0's logits: rows 0 and 5 see the same logits)."""
    forced = torch.full((6, max_len), -1, dtype=torch.long)
    forced[:, 0] = 31337                                              # column 0 is ignored, whatever it holds
    tok = lambda n: torch.randint(1000, 30000, (n,), generator=g)
    forced[1, 1:] = tok(max_len - 1)
    forced[1, -1] = EOS
    forced[2, 1:4] = tok(3)
    forced[3, 1:4] = tok(3)
    forced[3, 4] = EOS
    forced[3, 5:] = 777
    forced[4, 1:] = tok(max_len - 1)
    return forced


def _greedy_forced(lib, logits, st, t, forced_d, sf, eos=EOS):
    from vitcap_amd._lib import check
    B, max_len = st['ids'].shape
    check(lib.vitcap_greedy_step_forced(p(logits), logits.stride(0), V, p(st['ids']), p(st['unf']), p(st['sum_lp']), p(st['cnt']),
                                        p(st['logprob']), p(st['margin']), p(st['raw_last']), B, t, max_len, eos, PAD, p(forced_d),
                                        sf, p(st['tok_lp']), S()), 'greedy_step_forced')


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize('sf', [0, 1])
def test_greedy_step_forced_rule(ops, sf):
    """vitcap_greedy_step_forced on synthetic logits, 19 steps, the six row kinds, both modes: ids / unfinished / cnt / raw_last
    exact, sum_lp / logprob / token_logprobs within 2e-5 of the restated rule; the margin tap is the free choice's top-2 margin;
    forcing the argmax (row 5) gives the free row's (row 0) values bit for bit."""
    from vitcap_amd._lib import lib
    B = 6
    g = torch.Generator().manual_seed(20 + sf)
    forced = _six_rows(g)
    st = _state(ops, B, LMAX)
    ref = Rule(B, LMAX, forced, sf)
    for t in range(1, LMAX):
        logits = torch.randn(B, VP, generator=g) * 2.0
        logits[:, V:] = 1e9                                           # padding columns must be ignored
        logits[:, EOS] = 14.0 if t == 15 else -10.0                   # step 15: every free row ends; forced rows take their token
        for b in range(1, 5):                                         # forced tokens are likely ones: |sum_lp| stays below 128, where
            if forced[b, t] >= 0 and forced[b, t] != EOS:             # 2e-5 is still more than two ulp of an fp32 sum
                logits[b, forced[b, t]] += 9.0
        logits[5] = logits[0]
        row = logits[:, :V]
        free = row.argmax(-1)
        forced[5, t] = free[0]
        live = ref.unf.bool()
        _greedy_forced(lib, logits.cuda(), st, t, forced.cuda(), sf)
        top2 = torch.topk(row, 2).values
        assert torch.equal(st['margin'][:, t].cpu()[live], (top2[:, 0] - top2[:, 1])[live]), t
        ref.step(t, free, torch.log_softmax(row.double(), -1))
    worst = ref.check(st, 'greedy_step_forced sf=%d' % sf)
    print('MEASURED greedy_step_forced sf=%d: max |log-prob - rule| %.3e' % (sf, worst))
    ids = ref.ids
    assert ids[0, 15] == EOS and ids[0, 16:].eq(PAD).all()            # free row: ended by its own choice
    assert ids[1].tolist() == [BOS] + forced[1, 1:].tolist() and int(ref.raw_last[1]) == EOS
    assert ids[2, 1:4].tolist() == forced[2, 1:4].tolist() and ids[2, 15] == EOS
    assert ids[3, 4] == EOS and ids[3, 5:].eq(PAD).all()              # the junk behind the forced end is ignored
    assert ids[4, 1:-1].tolist() == forced[4, 1:-1].tolist() and ids[4, -1] == EOS and int(ref.raw_last[4]) == int(forced[4, -1])
    assert torch.equal(ids[5], ids[0])
    tl, sl, lo = st['tok_lp'].cpu(), st['sum_lp'].cpu(), st['logprob'].cpu()
    assert torch.equal(tl[5], tl[0])                                  # the forced argmax is scored as the free choice, bit for bit
    if sf:
        assert sl[5] == sl[0] and lo[5] == lo[0] and float(st['cnt'][1]) == 19 and float(st['cnt'][3]) == 4
    else:
        assert float(st['cnt'][5]) == 0 and float(lo[5]) == 0.0 and float(lo[3]) == 0.0 and float(lo[1]) == 0.0
        assert float(st['cnt'][2]) == 12 and float(st['cnt'][0]) == 15


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize('sf', [0, 1])
def test_greedy_select_embed_forced_equals_step_plus_embed(ops, sf):
    """vitcap_greedy_select_embed_forced on the row statistics and logits of a real vocabulary GEMM: the tokens of
    vitcap_greedy_step_forced on the same logits, log-probs within 2e-5, and x rows == vitcap_embed_step of the tokens taken
    (the forced ones), bit for bit."""
    from vitcap_amd._lib import lib, check
    B = 6
    g = torch.Generator().manual_seed(7 + sf)
    bf = lambda x: x.to(torch.bfloat16)
    wl = torch.zeros(VP, 768)
    wl[:V] = torch.randn(V, 768, generator=g) * 0.05
    wl = bf(wl).cuda()
    bias = torch.full((VP,), -1e30)
    bias[:V] = torch.randn(V, generator=g)
    word = bf(torch.randn(VP, 768, generator=g) * 0.05).cuda()
    pos = bf(torch.randn(512, 768, generator=g) * 0.05).cuda()
    typ = bf(torch.randn(2, 768, generator=g) * 0.05).cuda()
    gam = (1 + torch.randn(768, generator=g) * 0.1).cuda()
    bet = (torch.randn(768, generator=g) * 0.1).cuda()
    forced = _six_rows(g)
    st_a, st_b = _state(ops, B, LMAX), _state(ops, B, LMAX)
    worst = 0.0
    for t in range(1, LMAX):
        h = bf(torch.randn(B, 768, generator=g))
        h[5] = h[0]
        bias_t = bias.clone()
        bias_t[EOS] = 20.0 if t == 15 else -10.0
        for b in range(1, 5):                                         # likely forced tokens (a column's bias serves every row): the
            if forced[b, t] >= 0 and forced[b, t] != EOS:             # sums of log-probs stay where 2e-5 is more than two fp32 ulp
                bias_t[forced[b, t]] += 8.0
        logits, rs = ops.gemm_rowstat(h.cuda(), wl, bias_t.cuda())
        forced[5, t] = int(logits[0, :V].argmax())
        fd = forced.cuda()
        _greedy_forced(lib, logits, st_a, t, fd, sf)
        lastp = t == LMAX - 1
        xf = None if lastp else torch.empty((2 * B, 768), device='cuda')
        xb = None if lastp else torch.empty((2 * B, 768), device='cuda', dtype=torch.bfloat16)
        check(lib.vitcap_greedy_select_embed_forced(p(rs), rs.shape[1], p(logits), logits.stride(0), V, p(st_b['ids']), p(st_b['unf']),
                                                    p(st_b['sum_lp']), p(st_b['cnt']), p(st_b['logprob']), p(st_b['raw_last']), B, t,
                                                    LMAX, EOS, PAD, 103, p(word), p(pos), p(typ), p(gam), p(bet), 1e-12, p(xf), p(xb),
                                                    p(fd), sf, p(st_b['tok_lp']), S()), 'greedy_select_embed_forced')
        assert torch.equal(st_a['ids'], st_b['ids']), t
        assert torch.equal(st_a['unf'], st_b['unf']) and torch.equal(st_a['cnt'], st_b['cnt'])
        for k in ('sum_lp', 'tok_lp'):
            err = float((st_a[k] - st_b[k]).abs().max())
            worst = max(worst, err)
            assert err <= LP_TOL, (t, k, err)
        if not lastp:
            want_f, want_b = ops.embed_step(st_b['ids'], t + 1, word, pos, typ, gam, bet)
            assert torch.equal(xf, want_f) and torch.equal(xb, want_b), t
    assert torch.equal(st_a['raw_last'], st_b['raw_last'])
    assert float((st_a['logprob'] - st_b['logprob']).abs().max()) <= LP_TOL
    ids = st_b['ids'].cpu()
    assert ids[1].tolist() == [BOS] + forced[1, 1:].tolist() and ids[3, 4] == EOS and ids[3, 5:].eq(PAD).all()
    assert ids[4, 1:-1].tolist() == forced[4, 1:-1].tolist() and torch.equal(ids[5], ids[0]) and ids[0, 15] == EOS
    assert torch.equal(st_b['tok_lp'][5], st_b['tok_lp'][0])
    print('MEASURED greedy_select_embed_forced sf=%d: max |log-prob - greedy_step_forced| %.3e' % (sf, worst))


# ------------------------------------------------------------------------------------------------ 3
def test_sample_step_forced(ops):
    """vitcap_sample_step_forced with top-k and top-p on: forced rows take their token with the UNFILTERED
    log_softmax(logits / temperature) (within 2e-5 of torch; the tokens are ones the filter removes), free rows and free steps of
    the same launches produce exactly what vitcap_sample_step_offset produces with the same seed and offset."""
    from vitcap_amd._lib import lib, check, SampleParams
    B, max_len, T, off = 6, 5, 0.7, 3
    sp = SampleParams(1, T, 40, 0.9, 41)
    g = torch.Generator().manual_seed(33)
    forced = torch.full((B, max_len), -1, dtype=torch.long)
    forced[1, 1:] = torch.randint(1000, 30000, (max_len - 1,), generator=g)
    forced[1, 3] = EOS                                                # row 1 ends at step 3 by a forced [SEP]
    forced[4, 2] = 12345                                              # row 4: one forced step between free ones
    fd = forced.cuda()
    st_f, st_x = _state(ops, B, max_len), _state(ops, B, max_len)
    ref = Rule(B, max_len, forced, 1)
    for t in range(1, max_len):
        logits = torch.randn(B, VP, generator=g) * 4.0
        logits[:, V:] = 1e9
        logits[:, EOS] = -40.0                                        # no free row ends: every free step stays comparable
        ld = logits.cuda()
        args = lambda st: (p(ld), VP, V, p(st['ids']), p(st['unf']), p(st['sum_lp']), p(st['cnt']), p(st['logprob']), p(st['margin']),
                           p(st['raw_last']), B, t, max_len, EOS, PAD, C.byref(sp), off)
        check(lib.vitcap_sample_step_offset(*args(st_x), S()), 'sample_step_offset')
        check(lib.vitcap_sample_step_forced(*args(st_f), p(fd), 1, p(st_f['tok_lp']), S()), 'sample_step_forced')
        x = (logits[:, :V] / T).double()
        filtered_out = x.gather(1, forced[:, t].clamp(min=0)[:, None])[:, 0] < torch.topk(x, 40).values[:, -1]
        assert bool(filtered_out[forced[:, t] >= 0].all()), 'the forced tokens of this test are ones top-k removes'
        ref.step(t, st_x['ids'][:, t].cpu(), torch.log_softmax(x, -1))
    got, base = st_f['ids'].cpu(), st_x['ids'].cpu()
    free_rows = [0, 2, 3, 5]
    assert torch.equal(got[free_rows], base[free_rows])
    assert torch.equal(st_f['logprob'].cpu()[free_rows], st_x['logprob'].cpu()[free_rows])       # same draws, same filter, same bits
    assert torch.equal(st_f['margin'].cpu()[free_rows], st_x['margin'].cpu()[free_rows])
    assert torch.equal(got[4, [1, 3, 4]], base[4, [1, 3, 4]]) and int(got[4, 2]) == 12345
    assert got[1].tolist() == [BOS] + forced[1, 1:3].tolist() + [EOS, PAD]
    assert torch.equal(got, ref.ids) and torch.equal(st_f['cnt'].cpu().double(), ref.cnt)
    assert float(st_f['margin'][1, 1]) == 0.0 and float(st_f['margin'][4, 2]) == 0.0
    fmask = forced >= 0
    fmask[1, 4] = False                                               # behind row 1's end
    err = (st_f['tok_lp'].cpu().double() - ref.tok_lp).abs()[fmask]
    print('MEASURED sample_step_forced: max |forced log-prob - torch| %.3e over %d forced steps' % (float(err.max()), int(fmask.sum())))
    assert float(err.max()) <= LP_TOL
    assert abs(float(st_f['logprob'][1]) - float(ref.logprob[1])) <= LP_TOL
    assert bool(torch.isfinite(st_f['tok_lp']).all())


# ------------------------------------------------------------------------------------------------ 4
def _greedy_opts(m, **over):
    return m.gen_options(num_beams=1, do_sample=False, num_return_sequences=1, num_keep_best=1, **over)


def _raw_generate_forced(m, img, o, forced=None, sf=0, want_tlp=False):
    """vitcap_engine_generate_forced called directly (model.run takes the plain entry point when nothing is forced)."""
    from vitcap_amd._lib import lib, check
    B = img.shape[0]
    ws, need = m._workspace(B, m._packed[2], 0, o)
    ids, lp = m._out_buffers(B, o, img.device)
    tlp = torch.empty((B * o.seqs_per_image, o.max_length), device=img.device) if want_tlp else None
    check(lib.vitcap_engine_generate_forced(m._engine, p(img), int(img.dtype == torch.bfloat16), B, C.byref(o), p(ws), need, p(forced),
                                            sf, p(ids), p(lp), p(tlp), None, None, S()), 'engine_generate_forced')
    return ids, lp, tlp


@pytest.mark.parametrize('B,over', [(4, {}), (5, {}), (4, {'decode_streams': 2}), (4, {'use_graph': True})])
def test_nothing_forced_is_bit_identical_to_plain_generate(model, B, over):
    """An all -1 array, a NULL forced pointer (with and without the per-token output) and the staged decode entry point
    vitcap_engine_decode_forced: ids and logprobs bit-identical to the plain generate call."""
    img = _images(B, 55).cuda()
    ids0, lp0 = model.generate(img, **over)
    o = _greedy_opts(model, **over)
    free = torch.full((B, LMAX), -1, dtype=torch.int64, device='cuda')
    runs = {'all -1': _raw_generate_forced(model, img, o, free, 1),
            'NULL, NULL': _raw_generate_forced(model, img, o, None, 0),
            'NULL + token_logprobs': _raw_generate_forced(model, img, o, None, 0, want_tlp=True),
            'all -1, prompt mode, token_logprobs': _raw_generate_forced(model, img, o, free, 0, want_tlp=True)}
    ids_d, lp_d, last_d, tlp_d = model.run(img, o, want_last=True, forced=free, score_forced=1, want_token_logprobs=True)
    runs['decode_forced'] = (ids_d, lp_d, tlp_d)
    for name, (ids, lp, tlp) in runs.items():
        assert torch.equal(ids, ids0) and torch.equal(lp, lp0), name
        if tlp is not None:
            assert bool((tlp[:, 0] == 0).all()) and torch.equal(tlp, tlp_d), name
    assert torch.equal(last_d, model.run(img, o, want_last=True)[2])


# ------------------------------------------------------------------------------------------------ 5
def _counted_mean(tlp, ids):
    """sum of token_logprobs over the positions a caption holds a token at (its end included) / their number, in float64"""
    n = (ids[:, 1:] != PAD).sum(1).double()
    return tlp[:, 1:].double().sum(1) / n, n


@pytest.mark.parametrize('eos_ids', [[EOS], None])
def test_own_output_forced_scores_as_the_free_run(model, eos_ids):
    """score() on generate()'s own captions: the same ids, logprob and token_logprobs within 2e-5 of the free run, and
    sum(token_logprobs over the counted positions) / cnt == logprob.  Second case: a second EOS id (a word of the captions) makes
    them end early, so that forced entries behind an end and frozen scores are covered."""
    img = _images(4, 56).cuda()
    over = {}
    if eos_ids is None:
        ids_plain, _ = model.generate(img)
        over = {'eos_token_ids': [EOS, int(ids_plain[0, 0, 7])]}
    o = _greedy_opts(model, **over)
    ids0, lp0, last0, tlp0 = model.run(img, o, want_last=True, want_token_logprobs=True)
    if eos_ids is None:
        ends = (ids0[:, 0] == over['eos_token_ids'][1]).any(1)
        assert bool(ends.any()), 'the second EOS id must end at least one caption early'
    for last_tok in (None, last0):
        lp1, tlp1, ids1 = model.score(img, ids0[:, 0], return_ids=True, last_tok=last_tok, **over)
        assert torch.equal(ids1, ids0)
        d_lp, d_tok = float((lp1 - lp0[:, 0]).abs().max()), float((tlp1 - tlp0).abs().max())
        print('MEASURED own output forced (eos %s, last_tok %s): max |d logprob| %.3e, max |d token_lp| %.3e'
              % (over.get('eos_token_ids', [EOS]), last_tok is not None, d_lp, d_tok))
        assert d_lp <= LP_TOL and d_tok <= LP_TOL
        mean, n = _counted_mean(tlp1.cpu(), ids1[:, 0].cpu())
        # fp32 running sum of <= 19 terms of magnitude < 16 against a float64 sum: <= 19 half-ulps of 2^8 = 2.9e-4 in the sum at the
        # very worst, 1.5e-5 after the division by 19; the kernel's running sum is sequential, so the typical error is far smaller
        assert float((mean - lp1.cpu().double()).abs().max()) <= 1.5e-5
        assert bool((tlp1[:, 0] == 0).all()) and bool((tlp1.cpu()[ids1[:, 0].cpu() == PAD] == 0).all())


# ------------------------------------------------------------------------------------------------ 6
def test_reference_goldens_scored_without_a_floor(model, golden):
    """score() on the reference's own ids (reference_population.npz: 2 x 16 images; the four greedy_sel images): the returned
    ids equal the forced ones and the sequence log-prob of EVERY image is within 1e-2 of the reference's -- no margin floor, no
    allow-list."""
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
        lp, tlp, ids = model.score(img.cuda(), want, return_ids=True)
        assert torch.equal(ids[:, 0].cpu(), want), name
        dev = np.abs(lp.cpu().numpy() - ref_lp[:, 0])
        worst[name] = float(dev.max())
        print('MEASURED %s: max |sequence log-prob - reference| %.3e (image %d), mean %.3e over %d images'
              % (name, dev.max(), int(dev.argmax()), dev.mean(), len(dev)))
    for name, w in worst.items():
        assert w <= SEQ_TOL, (name, w)


# ------------------------------------------------------------------------------------------------ 7
def test_token_logprobs_vs_fp32_oracle(model, sd_t):
    """B = 2: the oracle's fp32 greedy captions scored on the device; token_logprobs against log_softmax of the oracle's own
    logits rows (return_trace) within 4e-2.  The rms is printed (test_per_step_logits_vs_reference allows 4e-3 rms per logit)."""
    from oracle import vitcap_oracle as O
    img = _images(2, 1234)
    with torch.no_grad():
        ids_o, lp_o, tr = O.greedy_incremental(sd_t, img, return_trace=True)
    lp_tok = torch.zeros(2, LMAX, dtype=torch.float64)
    tok = ids_o[:, 0].clone()
    for t, stp in enumerate(tr['steps'], 1):
        if t == LMAX - 1:
            tok[:, t] = stp['logits_row'].argmax(-1)                  # what the oracle chose there (the ids hold the forced [SEP])
        lp_tok[:, t] = torch.log_softmax(stp['logits_row'].double(), -1).gather(1, tok[:, t:t + 1])[:, 0]
    assert not bool((ids_o[:, 0, 1:-1] == EOS).any()), 'the recipe\'s captions run to the last position'
    lp, tlp, ids = model.score(img.cuda(), ids_o[:, 0], return_ids=True, last_tok=tok[:, -1])
    assert torch.equal(ids.cpu(), ids_o)
    err = (tlp.cpu().double() - lp_tok)[:, 1:]
    print('MEASURED token_logprobs vs fp32 oracle: max %.3e, rms %.3e over %d tokens (per-logit rms bound of the logits test: 4e-3)'
          % (float(err.abs().max()), float(err.pow(2).mean().sqrt()), err.numel()))
    assert float(err.abs().max()) <= TOK_TOL
    assert float((lp.cpu() - lp_o[:, 0]).abs().max()) <= SEQ_TOL


# ------------------------------------------------------------------------------------------------ 8
PROMPT_SEED = 6           # gen_image_batch(4, 6): the oracle alone decides 44-46 of the 66 free decisions above the floor (checked
                          # on the CPU of two machines; seeds 1..9 give 24..44)
PROMPT_PREFIX = [[-1] * 6, [9138] + [-1] * 5, [9138, 14292, 2568] + [-1] * 3, [9138, 14292, 9138, 27024, 7086, 18218]]
PROMPT_LEN = [0, 1, 3, 6]


def test_prompt_mode_vs_emulating_oracle(model, sd_t):
    """generate(prefix_ids=...) with per-row prefix lengths 0 / 1 / 3 / 6 against the bf16-emulating oracle driven by the forced
    sampler: forced positions exact, free positions identical on each row's comparable prefix (the trace's margins, the greedy
    floor), logprob == the mean of the trace's log-probs over the FREE positions only, within 1e-2."""
    from oracle import vitcap_oracle as O
    from vitcap_amd.forced import pack_forced
    img = _images(4, PROMPT_SEED)
    forced, sf = pack_forced(prefix_ids=PROMPT_PREFIX, rows=4, max_length=LMAX)
    assert sf == 0
    with torch.no_grad():
        ids_o, _, tr = O.greedy_incremental(sd_t, img, emulate_bf16=True, return_trace=True, sampler=forced_sampler(forced))
    margins = torch.stack([s['margin'] for s in tr['steps']], 1).numpy().astype(np.float64)
    for b, P in enumerate(PROMPT_LEN):
        margins[b, :P] = np.inf                                       # a forced position is no decision
    total = comparable = 0
    for b, P in enumerate(PROMPT_LEN):
        n = comparable_prefix(relevant_margins(ids_o[b, 0].numpy(), margins[b], EOS), GREEDY_MARGIN_FLOOR)
        total, comparable = total + (LMAX - 1 - P), comparable + max(0, n - P)
    print('MEASURED prompt mode: %d of %d free decisions comparable' % (comparable, total))
    assert 2 * comparable >= total, 'condition: at least half of all free decisions must be comparable'
    ids, lp, tlp = model.generate(img.cuda(), prefix_ids=torch.tensor(PROMPT_PREFIX), want_token_logprobs=True)
    got = ids.cpu()
    for b, P in enumerate(PROMPT_LEN):
        assert got[b, 0, 1:1 + P].tolist() == PROMPT_PREFIX[b][:P], b
    rep = assert_tokens_match_reference(got.numpy(), ids_o.numpy(), margins, GREEDY_MARGIN_FLOOR, min_full=0, what='prompt mode')
    # the score: free positions only (a reference loop started at cur_len = P); compared where the whole caption is the oracle's
    same = [r[0] for r in rep if r[4]]
    assert len(same) >= 1, rep
    want = torch.zeros(4, dtype=torch.float64)
    for b, P in enumerate(PROMPT_LEN):
        lps = []
        for t in range(P + 1, LMAX):
            row = tr['steps'][t - 1]['logits_row'][b].double()
            tok = row.argmax() if t == LMAX - 1 else ids_o[b, 0, t]
            lps.append(torch.log_softmax(row, -1)[tok])
        want[b] = torch.stack(lps).mean()
    d = (lp[:, 0].cpu().double() - want).abs()[same]
    print('MEASURED prompt mode: max |logprob - oracle over free positions| %.3e on %d whole-caption rows' % (float(d.max()), len(same)))
    assert float(d.max()) <= SEQ_TOL
    # per token, on every row up to its first token that is not the oracle's: the logits of those steps come from equal prefixes
    worst = 0.0
    for b, P in enumerate(PROMPT_LEN):
        diff = (got[b, 0] != ids_o[b, 0]).nonzero()
        last = int(diff[0]) if len(diff) else LMAX - 2                # the last column holds the max-length [SEP], not the choice
        for t in range(1, min(last, LMAX - 2) + 1):
            lsm = torch.log_softmax(tr['steps'][t - 1]['logits_row'][b].double(), -1)
            worst = max(worst, abs(float(tlp[b, t]) - float(lsm[got[b, 0, t]])))
    print('MEASURED prompt mode: max |token_lp - emulating oracle| %.3e' % worst)
    assert worst <= TOK_TOL
    # the forced tokens are reported per token but not counted
    mean_free = torch.stack([tlp[b, 1 + P:].double().sum() / (LMAX - 1 - P) for b, P in enumerate(PROMPT_LEN)])
    assert float((mean_free.cpu() - lp[:, 0].cpu().double()).abs().max()) <= 1.5e-5
    assert bool((tlp[3, 1:7] != 0).all())


# ------------------------------------------------------------------------------------------------ 9
def test_three_captions_per_image_share_the_encoder(model):
    """seqs_per_image = 3: an image's three given captions share its encoder pass and visual K/V; against the same captions on
    the 3 x repeated batch: same ids, sequence log-probs within 1e-2 and token log-probs within 4e-2 (the shared-K/V attention
    kernel rounds differently)."""
    img = _images(2, 57).cuda()
    ids0, _ = model.generate(img)
    c = ids0[:, 0].cpu()
    caps = c.repeat_interleave(3, 0).clone()
    for i in range(2):
        caps[3 * i + 1, 3] = 2023 + i                                 # another word at position 3
        caps[3 * i + 2, 5] = 4000 + i                                 # another word at position 5 and an early end
        caps[3 * i + 2, 8] = EOS
        caps[3 * i + 2, 9:] = PAD
    lp3, tlp3, ids3 = model.score(img, caps, seqs_per_image=3, return_ids=True)
    lp1, tlp1, ids1 = model.score(img.repeat_interleave(3, 0).contiguous(), caps, return_ids=True)
    assert torch.equal(ids3, ids1) and torch.equal(ids3[:, 0].cpu(), caps)
    d_lp, d_tok = float((lp3 - lp1).abs().max()), float((tlp3 - tlp1).abs().max())
    print('MEASURED K=3 vs repeated batch: max |d logprob| %.3e, max |d token_lp| %.3e' % (d_lp, d_tok))
    assert d_lp <= SEQ_TOL and d_tok <= TOK_TOL
    assert float((lp3[0] - lp3[1]).abs()) > 1e-3                      # the three captions of an image are scored as different captions


# ------------------------------------------------------------------------------------------------ 10
def test_graph_replay_reads_this_calls_forced_ids(model):
    """use_graph = 1, two calls with different forced ids (and other output tensors) on one workspace: each equals its eager
    result bit for bit, and the second call replays the first call's graph."""
    img = _images(3, 58).cuda()
    ids0, _ = model.generate(img)
    a = ids0[:, 0].cpu().clone()
    b = a.clone()
    b[:, 2] = torch.tensor([2023, 2024, 2025])
    b[1, 6] = EOS
    b[1, 7:] = PAD
    eager = [model.score(img, c, return_ids=True) for c in (a, b)]
    assert not torch.equal(eager[0][0], eager[1][0])
    n0 = model.graph_count()
    replay = [model.score(img, c, return_ids=True, use_graph=True) for c in (a, b, a)]
    assert model.graph_count() == n0 + 1
    for got, want in zip(replay, eager + eager[:1]):
        for x, y in zip(got, want):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 11
def test_pipeline_caption_prefix(model, tmp_path, monkeypatch):
    """Config key caption_prefix: every caption of the predict TSV starts with the prefix text, is the caption
    generate(prefix_ids=...) gives, and the TSV columns are what they were (key, JSON list of {caption, conf})."""
    from vitcap_amd.pipeline import CaptionUniPipeline
    monkeypatch.chdir(tmp_path)
    enc = tmp_path / 'enc'
    enc.mkdir()
    toks = ['[PAD]'] + ['w%d' % i for i in range(1, 30522)]
    toks[100], toks[101], toks[102], toks[103] = '[UNK]', '[CLS]', '[SEP]', '[MASK]'
    (enc / 'vocab.txt').write_text('\n'.join(toks) + '\n')
    img = _images(2, 59)
    pipe = CaptionUniPipeline(full_expid='E', init_recipe_seed=0, text_encoder_type=str(enc), tagemb='cls', force_predict=True,
                              test_batches=[{'image': img.clone(), 'key': ['k0', 'k1']}], model_file=str(tmp_path / 'm.pt'),
                              caption_prefix='W14292 w9138')
    assert pipe.caption_prefix_ids() == [14292, 9138]
    out = pipe.ensure_predict()
    ids, lp = model.generate(img.cuda(), prefix_ids=torch.tensor([[14292, 9138]] * 2))
    plain, _ = model.generate(img.cuda())
    assert not torch.equal(plain[:, 0, 1:3], ids[:, 0, 1:3])
    rows = [l.rstrip('\n').split('\t') for l in open(out)]
    assert [r[0] for r in rows] == ['k0', 'k1'] and all(len(r) == 2 for r in rows)
    for i, r in enumerate(rows):
        rec = json.loads(r[1])
        assert len(rec) == 1 and set(rec[0]) == {'caption', 'conf'}
        assert rec[0]['caption'].startswith('w14292 w9138 ')
        assert rec[0]['caption'].split() == ['w%d' % int(t) for t in ids[i, 0, 1:] if int(t) not in (PAD, BOS, EOS)]
        assert abs(rec[0]['conf'] - float(torch.exp(lp[i, 0]))) < 1e-6
