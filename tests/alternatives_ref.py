"""The row rule of the token alternatives (include/vitcap_hip.h: vitcap_score_rows_alts), restated in float64 on fp32 rows, and a
generator of planted rows.  Shared by tests/test_alternatives_cpu.py (which checks the restatement against independent torch formulas)
and tests/test_hip_alternatives.py (which checks the kernel against the restatement).

For caption c and position t in 1 .. L-1, x = the probe row's V fp32 logits:
  live      no EOS id (eos or one of eos_extra) among cap[1 .. t-1]
  f         the given token when it lies inside the vocabulary, else the row's argmax; in the last column a written [SEP] is
            replaced by last_tok[c] when that is an id of the vocabulary, else by the argmax
  order     i before j iff x[i] > x[j], or x[i] == x[j] and i < j (float comparison: -0.0 == +0.0)
  alt_ids   the first k indices of the order;  alt_lp = (x[id] - m) - log S, m = max x, S = sum exp(x - m)
  rank      the number of entries that come before f
  entropy   log S - T / S, T = sum exp(x - m) (x - m)
Dead rows and column 0: alt_ids = rank = -1, alt_lp = entropy = 0."""
import numpy as np

EOS, PAD, BOS = 102, 0, 101
LP_TOL = 2e-5                      # |alt_lp - float64|: the bound tests/test_hip_forced.py 1-3 use for this arithmetic
ENT_ULPS = 64                      # 30 serial + 10 tree additions on an element's path, a few ulp of expf / logf, rounded up
# The rule's terms are e_i = expf(x_i - m), an fp32 function: below 2^-150 it returns 0.  The restatement keeps that range (not the
# rounding): a term that is zero in the rule is zero here, so that a dominated row has S = 1, T = 0 and entropy 0 in both.  The rows of
# the tests stay out of fp32's subnormal range (-103.97 < x - m < -87.3), where expf has a few bits only.
EXPF_ZERO = -150 * np.log(2.0)
PLANTED = ('argmax', 'worst', 'tie_lower', 'tie_higher', 'zeros', 'all_equal', 'dominated', 'random')


def order(x):
    """Indices of the fp32 row x in the order of the rule.  np.lexsort compares -0.0 and +0.0 as equal; the index breaks ties."""
    x = np.asarray(x, dtype=np.float32)
    return np.lexsort((np.arange(x.shape[0]), -x.astype(np.float64)))


def row_ref(x, f, k):
    """One live row -> dict(ids (k,), lp (k,) f64, rank, entropy f64, ent_tol, lp_f f64): the table of the rule."""
    x32 = np.asarray(x, dtype=np.float32)
    x64 = x32.astype(np.float64)
    m = x64.max()
    d = x64 - m
    e = np.where(d < EXPF_ZERO, 0.0, np.exp(d))
    S, T = e.sum(), (e * d).sum()
    ids = order(x32)[:k]
    idx = np.arange(x32.shape[0])
    rank = int(((x32 > x32[f]) | ((x32 == x32[f]) & (idx < f))).sum())
    logS = np.log(S)
    return dict(ids=ids.astype(np.int32), lp=d[ids] - logS, rank=rank, entropy=logS - T / S,
                ent_tol=ENT_ULPS * 2.0 ** -24 * (abs(logS) + abs(T) / S), lp_f=d[f] - logS)


def is_eos(tok, eos=EOS, eos_extra=()):
    return int(tok) == eos or int(tok) in [int(e) for e in eos_extra]


def live_rows(ids, eos=EOS, eos_extra=()):
    """(n_caps, L) int64 -> bool (n_caps, L): position t >= 1 is live while no EOS id lies among cap[1 .. t-1]; column 0 never."""
    ids = np.asarray(ids)
    live = np.zeros(ids.shape, dtype=bool)
    for c in range(ids.shape[0]):
        ended = False
        for t in range(1, ids.shape[1]):
            live[c, t] = not ended
            ended = ended or is_eos(ids[c, t], eos, eos_extra)
    return live


def scored_token(x, cap, t, last_tok_c, V, eos=EOS):
    """f of the rule for a live row."""
    L = len(cap)
    amax = int(order(x)[0])
    given = int(cap[t])
    f = given if 0 <= given < V else amax
    if t == L - 1 and given == eos:
        lt = -1 if last_tok_c is None else int(last_tok_c)
        f = lt if 0 <= lt < V else amax
    return f


def alternatives_ref(logits, V, ids, k, rows0=0, last_tok=None, eos=EOS, eos_extra=()):
    """logits fp32 (n_rows, >= V): the probe rows [rows0, rows0 + n_rows) of captions ids (n_caps, L).  -> dict of
    ids int32 (n_caps, L, k), lp f64 (n_caps, L, k), rank int32 (n_caps, L), entropy f64, ent_tol f64, f int64 (-1 where none),
    lp_f f64 (the scored token's log-prob), covered bool (n_caps, L): the positions the call writes, live bool."""
    logits = np.asarray(logits, dtype=np.float32)
    ids = np.asarray(ids)
    n_caps, L = ids.shape
    live = live_rows(ids, eos, eos_extra)
    out = dict(ids=np.full((n_caps, L, k), -1, np.int32), lp=np.zeros((n_caps, L, k)), rank=np.full((n_caps, L), -1, np.int32),
               entropy=np.zeros((n_caps, L)), ent_tol=np.zeros((n_caps, L)), f=np.full((n_caps, L), -1, np.int64),
               lp_f=np.zeros((n_caps, L)), covered=np.zeros((n_caps, L), bool), live=live)
    for r in range(logits.shape[0]):
        g = rows0 + r
        c, t = g // (L - 1), g % (L - 1) + 1
        out['covered'][c, t] = True
        if not live[c, t]:
            continue
        x = logits[r, :V]
        f = scored_token(x, ids[c], t, None if last_tok is None else last_tok[c], V, eos)
        w = row_ref(x, f, k)
        out['ids'][c, t], out['lp'][c, t], out['rank'][c, t] = w['ids'], w['lp'], w['rank']
        out['entropy'][c, t], out['ent_tol'][c, t], out['f'][c, t], out['lp_f'][c, t] = w['entropy'], w['ent_tol'], f, w['lp_f']
    return out


def planted_rows(V, seed, ld=None):
    """The eight rows of PLANTED for a vocabulary of V (>= 16) entries -> (logits fp32 (8, ld) with the columns behind V set to
    1e9 -- they must be ignored --, f (8,) the token each row is to be scored on; never EOS)."""
    assert V >= 16
    rng = np.random.RandomState(seed)
    ld = V if ld is None else ld
    x = (rng.randn(8, V) * 2.0).astype(np.float32)
    f = np.zeros(8, np.int64)
    hi, lo = min(V - 1, 900), 3
    # argmax: f is the row's only maximum
    f[0] = V - 2
    x[0, f[0]] = 30.0
    # worst: f is the last entry of the order: the minimum, tied with a LOWER index, so rank is V - 1
    f[1] = V - 1
    x[1, f[1]] = -40.0
    x[1, lo] = -40.0
    # f tied with a lower index (which comes first) / with a higher one (which comes after), at the top of the row
    f[2] = hi
    x[2, hi] = x[2, lo] = 25.0
    f[3] = lo
    x[3, hi] = x[3, lo] = 25.0
    # a +0 / -0 pair on top of a negative row: -0.0 at the lower index comes first, the +0.0 second; f is the +0.0
    x[4] = -np.abs(x[4]) - 1.0
    x[4, lo], x[4, hi] = -0.0, 0.0
    f[4] = hi
    # all equal: entropy ln V, rank = the index
    x[5] = np.float32(1.25)
    f[5] = V // 2
    # one entry dominates: every other exp underflows in fp32 (and S = 1 exactly)
    x[6, 7] = 120.0
    f[6] = 9
    # a plain random row, f anywhere
    f[7] = int(rng.randint(0, V))
    f[f == EOS] += 1
    out = np.full((8, ld), 1e9, np.float32)
    out[:, :V] = x
    return out, f
