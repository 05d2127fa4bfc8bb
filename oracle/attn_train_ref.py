"""fp64 reference of the training attention (forward + backward over packed qkv) with per-element error bounds, the
visibility rule of vitcap_amd/csrc/common.h written out once more, deliberately wrong variants of it, and inputs on
which a single wrong (query, key) decision moves a whole row.  Plain torch on the CPU; nothing here touches the device
library.  Used by tests/test_attn_train_edges_cpu.py and tests/test_hip_attn_train_edges.py; the derivations are in
docs/LAB_tests_attn_train_edges.md.
"""
import numpy as np
import torch

HEADS, HD = 12, 64
U = 2.0 ** -8                      # unit roundoff of bf16 as the bounds count it (one ulp of a value in [1, 2) is 2^-7)

MASK_MUTATIONS = ('diag', 'causal+1', 'cf+1', 'cf-1', 'mf+1', 'mf-1', 'probe-1', 'probe+1', 'noself', 'probecausal',
                  'lastkey', 'pastend')
DATA_MUTATIONS = ('image-1', 'drop-shift', 'drop-T')


def visible(S, cf, mf, mutation=None):
    """(S, S) bool, [q, k]: may query row q attend key row k.  Rows are [0, cf) visual | [cf, mf) caption tokens |
    [mf, S) [MASK] probes; mf = 0: no probes, cf = 0: no mask at all.
      keys below cf are visible to everyone; a token key is visible causally (k <= q); a probe key only to itself;
      probe q sees the token keys with k - cf <= q - mf; and k < S.
    `mutation` (one of MASK_MUTATIONS) builds one deliberate error into the rule.  'pastend' is no visibility error but
    a key counted twice, so its result is uint8 with 2 in the last key's column: reference() reads a mask as the
    multiplicity of each key."""
    assert mutation is None or mutation in MASK_MUTATIONS, mutation
    q = torch.arange(S)[:, None].expand(S, S)
    k = torch.arange(S)[None, :].expand(S, S)
    d_cf = {'cf+1': 1, 'cf-1': -1}.get(mutation, 0)
    m = mf + {'mf+1': 1, 'mf-1': -1}.get(mutation, 0) if mf > 0 else 0
    plain = (k < cf + d_cf) if cf > 0 else torch.ones(S, S, dtype=torch.bool)
    if mutation == 'diag':
        causal = k < q
    elif mutation == 'causal+1':
        causal = k <= q + 1
    else:
        causal = k <= q
    probe_q = (q >= m) if m > 0 else torch.zeros(S, S, dtype=torch.bool)
    probe_k = (k >= m) if m > 0 else torch.zeros(S, S, dtype=torch.bool)
    slack = {'probe-1': -1, 'probe+1': 1}.get(mutation, 0)
    probe_rule = (k - cf) <= (q - m) + slack
    if mutation == 'noself':
        self_rule = torch.zeros(S, S, dtype=torch.bool)
    elif mutation == 'probecausal':
        self_rule = k <= q
    else:
        self_rule = k == q
    text = torch.where(probe_k, self_rule, torch.where(probe_q, probe_rule, causal))
    in_range = k < (S - 1 if mutation == 'lastkey' else S)
    vis = in_range & (plain | text)
    if mutation == 'pastend':
        vis = vis.to(torch.uint8)
        vis[:, S - 1] *= 2
    return vis


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def planted_inputs(B, S, cf, mf, seed, amp=1.5, a=1.4):
    """bf16 qkv (B, S, 2304) and dout (B, S, 768): uniform random like the existing attention tests, except that in
    heads 0..5 key rows are a * Q[q] * 48 / |Q[q]|^2 of a related query q, so that q's scaled score against that key is
    6a (8.4) above a field of standard deviation ~0.75 and its softmax sits on that one key whenever the key is visible:
      head 0: k = q;  head 1: k = q + 1;  head 2: k = q - 1;
      head 3: probe q = mf + j -> token key cf + j (the last it may see);
      head 4: probe q = mf + j -> token key cf + j + 1 (the first it may not see);
      head 5: key S-1 is scaled so that it takes 0.2 of row S-1, and V[S-1] = amp * sign(dout[S-1]), so that dP of that key
              stands far from the row's mean: a key counted twice then moves dS of the row by far more than its bound
              (at 0.4 it would not: P (1 - P) is the same at 0.4 and at the 0.57 the doubled key takes);
      head 6: the queries of the probes behind the first are built for key mf, which none of them may see."""
    qkv = _rand((B, S, 2304), seed, amp).to(torch.bfloat16)
    dout = _rand((B, S, 768), seed + 1, 1.0).to(torch.bfloat16)
    x = qkv.view(B, S, 3, HEADS, HD)
    Q = x[:, :, 0].double()
    want = a * Q * 48.0 / (Q * Q).sum(-1, keepdim=True)           # (B, S, 12, 64): the key that query row wants
    K = x[:, :, 1]
    K[:, :, 0] = want[:, :, 0].to(torch.bfloat16)
    if S > 1:
        K[:, 1:, 1] = want[:, :-1, 1].to(torch.bfloat16)
        K[:, :-1, 2] = want[:, 1:, 2].to(torch.bfloat16)
    if mf > 0:
        for j in range(S - mf):
            if cf + j < mf:
                K[:, cf + j, 3] = want[:, mf + j, 3].to(torch.bfloat16)
            if cf + j + 1 < mf:
                K[:, cf + j + 1, 4] = want[:, mf + j, 4].to(torch.bfloat16)
        if mf + 1 < S:                                            # head 6: the QUERIES are built, for one key
            Km = K[:, mf, 6].double()
            x[:, mf + 1:, 0, 6] = (a * Km * 48.0 / (Km * Km).sum(-1, keepdim=True))[:, None].to(torch.bfloat16)
    if S > 1:                                                     # head 5: 0.2 of row S-1 on key S-1, dP there far from the row's mean
        vis = visible(S, cf, mf)[S - 1].clone()
        vis[S - 1] = False
        s = 0.125 * (K[:, :, 5].double() * Q[:, S - 1:S, 5]).sum(-1)               # (B, S)
        t = torch.log(0.25 * torch.exp(s)[:, vis].sum(-1))
        K[:, S - 1, 5] = (t[:, None] / 6.0 * want[:, S - 1, 5] / a).to(torch.bfloat16)
        d5 = dout.view(B, S, HEADS, HD)[:, S - 1, 5]
        x[:, S - 1, 2, 5] = torch.where(d5 < 0, -amp, amp).to(torch.bfloat16)
    return qkv, dout


def dropout_keep(seed, B, S, p):
    """(B, 12, S, S) bool keep decisions of the device's counter hash (oracle.vitcap_oracle.dropout_keep)."""
    from oracle import vitcap_oracle as O
    return torch.from_numpy(O.dropout_keep(seed, B, S, p))


def mutate_data(qkv, keep, mutation):
    """The three data-path errors: (qkv', keep')."""
    assert mutation in DATA_MUTATIONS, mutation
    if mutation == 'image-1':                                     # image b reads image b-1's K / V
        x = qkv.clone()
        x[..., 768:] = torch.roll(qkv[..., 768:], 1, 0)
        return x, keep
    if mutation == 'drop-shift':                                  # the decision of key k-1 applied to key k
        return qkv, torch.roll(keep, 1, -1)
    return qkv, keep.transpose(-1, -2)                            # drop-T: query and key swapped in the hash


def reference(qkv, dout, mask, keep=None, p=0.0, scale=0.125, extra=None, heads=None):
    """fp64 forward and backward of softmax(scale q k^T + mask) [dropout] v per head, and bounds on what kernels with the
    device's rounding points (P, dS, the outputs in bf16; sums in fp32) may be off by.
      qkv (B, S, 2304), dout (B, S, 768), mask (S, S) multiplicity of key k for query q (bool or small integers),
      keep (B, 12, S, S) bool with p > 0, extra (B, S, 1536) = [dK | dV] added to dk / dv, heads: a subset to compute.
    Returns a dict: out, dq, dk, dv (B, S, H*64), lse2 (B, H, S) in the log2 domain, and b_out, b_dq, b_dk, b_dv."""
    B, S = qkv.shape[:2]
    hs = list(range(HEADS)) if heads is None else list(heads)
    H = len(hs)
    x = qkv.double().view(B, S, 3, HEADS, HD)[:, :, :, hs]
    do_all = dout.double().view(B, S, HEADS, HD)[:, :, hs]
    ex = extra.double().view(B, S, 2, HEADS, HD)[:, :, :, hs] if extra is not None else None
    w = mask.double()
    neg = torch.zeros(S, S, dtype=torch.float64).masked_fill(w == 0, float('-inf'))
    r = 1.0 / (1.0 - p) if p > 0 else 1.0
    res = {n: torch.empty(B, S, H, HD, dtype=torch.float64) for n in ('out', 'dq', 'dk', 'dv', 'b_out', 'b_dq', 'b_dk', 'b_dv')}
    res['lse2'] = torch.empty(B, H, S, dtype=torch.float64)
    for b in range(B):
        Q, K, V = (x[b, :, i].transpose(0, 1) for i in range(3))                 # (H, S, 64)
        dO = do_all[b].transpose(0, 1)
        s = Q @ K.transpose(-1, -2) * scale + neg
        mx = s.max(-1, keepdim=True).values
        e = torch.exp(s - mx) * w
        l = e.sum(-1, keepdim=True)
        P = e / l
        res['lse2'][b] = ((mx + torch.log(l)) / np.log(2.0)).squeeze(-1)
        kp = keep[b, hs].double() * r if p > 0 else None
        Ph = P * kp if p > 0 else P                                              # dropout-scaled P
        out = Ph @ V
        b_out = 2 * U * (Ph @ V.abs()) + 2 * U * out.abs()
        dPh = dO @ V.transpose(-1, -2)
        dP = dPh * kp if p > 0 else dPh
        D = (dO * out).sum(-1, keepdim=True)
        dS = P * (dP - D)
        dD = (dO.abs() * b_out).sum(-1, keepdim=True)
        ddS = 2 * U * dS.abs() + P * dD
        dq = scale * (dS @ K)
        dk = scale * (dS.transpose(-1, -2) @ Q)
        dv = Ph.transpose(-1, -2) @ dO
        b_dq = scale * (ddS @ K.abs()) + U * dq.abs()
        b_dk = scale * (ddS.transpose(-1, -2) @ Q.abs())
        b_dv = 2 * U * (Ph.transpose(-1, -2) @ dO.abs())
        if ex is not None:
            dk = dk + ex[b, :, 0].transpose(0, 1)
            dv = dv + ex[b, :, 1].transpose(0, 1)
        b_dk = b_dk + U * dk.abs()
        b_dv = b_dv + U * dv.abs()
        for n, t in (('out', out), ('dq', dq), ('dk', dk), ('dv', dv), ('b_out', b_out), ('b_dq', b_dq), ('b_dk', b_dk), ('b_dv', b_dv)):
            res[n][b] = t.transpose(0, 1)
    for n in list(res):
        if n != 'lse2':
            res[n] = res[n].reshape(B, S, H * HD)
    return res


def lse_bound(lse2):
    """The project's own tolerance on the log2-domain logsumexp (tests/test_hip_ops.py test_attn_dense_backward: 1e-4
    relative + 1e-3 absolute) plus the one term it lacks on rows that sit on a single key: the forward's row sum is
    the sum of the bf16-ROUNDED probabilities (attn.hip: the normaliser the numerator uses), each within u = 2^-8 of its
    value, so the sum lies within a factor 1 +- u of the exact one and lse2 within -log2(1 - u) = 5.65e-3.  Over
    a flat row those errors average out, which is why the existing tests never needed the term."""
    return 1e-4 * lse2.abs() + 1e-3 - np.log2(1.0 - U)


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def emulate(qkv, dout, mask, keep=None, p=0.0, scale=0.125, extra=None, heads=None):
    """What kernels with the device's rounding points compute, in fp64 between them: P = exp2(s c - ceil(max s c)) rounded
    to bf16 for the product and for the row sum, out rounded, lse2 from the rounded sum; the backward on THAT out and
    lse2 with P and dS rounded for the products and every output rounded once.  Not a second reference: it only tells,
    without a GPU, whether the bounds of reference() leave room for the rounding they were derived from."""
    B, S = qkv.shape[:2]
    hs = list(range(HEADS)) if heads is None else list(heads)
    H = len(hs)
    x = qkv.double().view(B, S, 3, HEADS, HD)[:, :, :, hs]
    do_all = dout.double().view(B, S, HEADS, HD)[:, :, hs]
    ex = extra.double().view(B, S, 2, HEADS, HD)[:, :, :, hs] if extra is not None else None
    w = mask.double()
    neg = torch.zeros(S, S, dtype=torch.float64).masked_fill(w == 0, float('-inf'))
    r = 1.0 / (1.0 - p) if p > 0 else 1.0
    c = scale * 1.4426950408889634
    res = {n: torch.empty(B, S, H, HD, dtype=torch.float64) for n in ('out', 'dq', 'dk', 'dv')}
    res['lse2'] = torch.empty(B, H, S, dtype=torch.float64)
    for b in range(B):
        Q, K, V = (x[b, :, i].transpose(0, 1) for i in range(3))
        dO = do_all[b].transpose(0, 1)
        s2 = Q @ K.transpose(-1, -2) * c + neg
        m = torch.ceil(s2.max(-1, keepdim=True).values)
        pb = _bf(torch.exp2(s2 - m)) * w
        l = pb.sum(-1, keepdim=True)
        kp = keep[b, hs].double() if p > 0 else None
        out = _bf(((pb * kp if p > 0 else pb) @ V) * (r / l))
        L = (m + torch.log2(l)).float().double()
        res['lse2'][b] = L.squeeze(-1)
        P = torch.exp2(s2 - L) * w
        dP = dO @ V.transpose(-1, -2)
        if p > 0:
            dP = dP * kp * r
        D = (dO * out).sum(-1, keepdim=True)
        dS = _bf(P * (dP - D))
        Pd = _bf(P) * kp if p > 0 else _bf(P)
        dk = scale * (dS.transpose(-1, -2) @ Q)
        dv = r * (Pd.transpose(-1, -2) @ dO)
        if ex is not None:
            dk = dk + ex[b, :, 0].transpose(0, 1)
            dv = dv + ex[b, :, 1].transpose(0, 1)
        for n, t in (('out', out), ('dq', _bf(scale * (dS @ K))), ('dk', _bf(dk)), ('dv', _bf(dv))):
            res[n][b] = t.transpose(0, 1)
    for n in list(res):
        if n != 'lse2':
            res[n] = res[n].reshape(B, S, H * HD)
    return res


# (B, S, ld_rows, cf, mf, p_drop, q_range): the edge cases of the training attention kernels, one table for the GPU parity
# test and for the CPU test that the planted inputs let no mutation hide (reasons: docs/LAB_tests_attn_train_edges.md)
CASES = [
    (1, 5, 5, 0, 0, 0.0, None),
    (2, 64, 64, 0, 0, 0.0, None),
    (2, 72, 80, 0, 0, 0.0, None),
    (2, 73, 73, 0, 0, 0.0, None),
    (1, 128, 128, 0, 0, 0.0, None),
    (3, 129, 136, 0, 0, 0.0, None),
    (1, 200, 200, 0, 0, 0.0, None),
    (1, 276, 276, 0, 0, 0.0, None),
    (2, 577, 577, 0, 0, 0.0, None),
    (2, 577, 577, 0, 0, 0.0, (0, 1)),
    (1, 1023, 1023, 0, 0, 0.0, None),
    (2, 200, 256, 0, 0, 0.0, (0, 70)),
    (2, 200, 256, 0, 0, 0.0, (128, 200)),
    (2, 598, 598, 578, 0, 0.0, None),
    (2, 598, 598, 578, 0, 0.1, None),
    (2, 598, 598, 578, 0, 0.0, (512, 598)),
    (2, 598, 598, 578, 0, 0.1, (512, 598)),
    (2, 598, 640, 576, 0, 0.0, None),
    (1, 598, 598, 598, 0, 0.0, None),
    (2, 580, 580, 578, 0, 0.0, None),
    (1, 580, 580, 580, 0, 0.0, None),
    (1, 577, 577, 576, 0, 0.0, None),
    (2, 617, 617, 578, 598, 0.0, None),
    (2, 617, 617, 578, 598, 0.1, None),
    (2, 617, 617, 578, 598, 0.0, (512, 617)),
    (2, 617, 617, 578, 598, 0.1, (512, 617)),
    (1, 639, 639, 578, 609, 0.0, None),
    (1, 598, 598, 578, 579, 0.0, None),
    (1, 598, 598, 578, 598, 0.0, None),
    (2, 100, 100, 70, 85, 0.0, None),
    (2, 40, 40, 10, 25, 0.0, None),
    (1, 130, 130, 128, 0, 0.0, (128, 130)),
]
DROP_SEED = 0x51f2ab17


def case_id(case):
    B, S, ld, cf, mf, p, qr = case
    return 'B%d-S%d-ld%d-cf%d-mf%d-p%g-%s' % (B, S, ld, cf, mf, p, 'all' if qr is None else 'q%d_%d' % qr)


def case_inputs(case):
    """(qkv, dout, keep) of a case: planted inputs seeded by the shape, dout zero outside the query range (the documented
    contract of the row-restricted entry points), the device's keep decisions with p > 0."""
    B, S, ld, cf, mf, p, qr = case
    qkv, dout = planted_inputs(B, S, cf, mf, seed=1000 + S + 7 * cf + 13 * mf)
    if qr is not None:
        dout[:, :qr[0]] = 0
        dout[:, qr[1]:] = 0
    keep = dropout_keep(DROP_SEED, B, S, p) if p > 0 else None
    return qkv, dout, keep


def covered_rows(S, qr):
    """Query rows the row-restricted forward and dQ write: the 128-row blocks covering the range."""
    lo, hi = (0, S) if qr is None else qr
    return lo, min(S, (hi + 127) // 128 * 128)
