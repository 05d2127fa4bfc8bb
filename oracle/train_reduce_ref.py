"""fp64 references of the kernels that close the training step -- LayerNorm forward / split-K LayerNorm / LayerNorm backward, the
bf16 cast with column sums, the three losses, the gradient norm and the fused clip + AdamW -- each with per-element error bounds
derived from the kernel's rounding points, deliberately wrong variants (`mutant=`) and the case tables.  Plain torch fp64 on the CPU;
nothing here touches the device library.  Used by tests/test_train_reduce_cpu.py and tests/test_hip_train_reduce.py; the derivations
are in docs/LAB_tests_train_reduce.md.

Every reference starts from the SAME fp32 / bf16 values the device gets (scalars such as eps, lr, b1 included: f32()), computes in fp64
and returns, next to each result, an array `b_<name>`: the bound on |device - reference| of that element.  A bound is a sum of terms
`count * E * magnitude` (E = 2^-24, one fp32 rounding; U = 2^-8, one bf16 rounding), the count being the roundings on the longest
chain that produces the element; expf, logf, log1pf, sqrtf and the division are budgeted at LIBM = 4 E relative per call.
"""
import math

import numpy as np
import torch

U = 2.0 ** -8            # one rounding to bf16 (8 significant bits, round to nearest)
E = 2.0 ** -24           # one rounding to fp32
TINY = 2.0 ** -126       # the smallest normal fp32: what a result below it may lose whichever way denormals are handled
LIBM = 4                 # roundings budgeted per expf / logf / log1pf / sqrtf / division
D = 768
NW = 8                   # waves per workgroup of layernorm_bwd_kernel / cast_bf16_colsum_kernel
DEFAULT_CUS = 256        # CPU-side stand-in for multi_processor_count; the GPU file passes the device's own


def f32(v):
    """The fp32 value of a Python scalar, as an fp64 number: what the device receives through a `float` argument."""
    return float(np.float32(v))


def rne_bf16(t):
    """Round-to-nearest-even of fp32 values to bf16, returned in fp32."""
    assert t.dtype == torch.float32
    return t.to(torch.bfloat16).to(torch.float32)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, std=1.0, mean=0.0):
    return torch.randn(shape, generator=_gen(seed)) * std + mean


def _uni(shape, seed, scale=1.0):
    return (torch.rand(shape, generator=_gen(seed)) * 2 - 1) * scale


# =====================================================================================================================
# LayerNorm: statistics shared by the forward and the backward
# =====================================================================================================================
# mean: 12 values per lane as three (a + b) + (c + d) added to s (longest chain 2 + 3), 6 butterfly steps, the product with 1/768
# and the rounding of that constant: 13 roundings, each relative to a partial sum <= sum |x|.
C_MEAN = 13
# variance: d = x - mean and d * d (3 roundings relative to the term), 12 accumulations in the lane, 6 butterfly steps, the product
# with 1/768 and the constant: 23
C_VAR = 23

LN_KINDS = ('ordinary', 'mean1000', 'zero', 'constant', 'spike', 'tiny', 'huge')


def ln_rows(M, seed, first_kind=None):
    """fp32 (M, 768): row r is of kind LN_KINDS[(r + first) % 7], first = M % 7 unless given, so that the small M of the case table
    see every kind between them.  ordinary N(0.5, 3) | mean 1000, std 0.01 | all zero | constant 7.3 | one 1e4 among zeros |
    magnitudes 1e-20 | magnitudes 1e15."""
    first = M % 7 if first_kind is None else first_kind
    x = _randn((M, D), seed, 3.0, 0.5)
    z = _randn((M, D), seed + 1)
    kind = (torch.arange(M) + first) % 7
    for k, name in enumerate(LN_KINDS):
        rows = (kind == k).nonzero().flatten()
        if name == 'mean1000':
            x[rows] = 1000.0 + 0.01 * z[rows]
        elif name == 'zero':
            x[rows] = 0.0
        elif name == 'constant':
            x[rows] = 7.3
        elif name == 'spike':
            x[rows] = 0.0
            x[rows, (rows * 37 + 5) % D] = 1e4
        elif name == 'tiny':
            x[rows] = 1e-20 * z[rows]
        elif name == 'huge':
            x[rows] = 1e15 * z[rows]
    return x.float(), kind


def ln_params(seed):
    """gamma 1 + U(-0.2, 0.2) with one negative and one zero entry, beta U(-1, 1) with one zero entry."""
    g = 1 + _uni((D,), seed, 0.2)
    b = _uni((D,), seed + 1, 1.0)
    g[5], g[300], b[17] = -0.7, 0.0, 0.0
    return g.float(), b.float()


def ln_stats(x, eps, mutant=None, dx_in=None):
    """mean, rstd, xhat of fp32 rows in fp64 with the bound d_xhat on the device's xhat.
      d_mean = C_MEAN E mean|x|;  the device's centred values are all shifted by its error of the mean, which adds d_mean^2 to its
      variance (the cross term vanishes) on top of C_VAR E var of rounding: rr = relative error of rstd =
      min(d_mean^2 / 2(var + eps), 1) + (C_VAR E var + TINY) / 2(var + eps) + 9 E  (var + eps, sqrtf, the division);
      d_xhat = rstd d_mean + |xhat| (2 E + rr)   (the rounding of x - mean and of the product with rstd).
    dx_in: bound on a perturbation of the INPUT (the split-K sum with activation), propagated to first order."""
    x = x.double()
    eps = f32(eps)
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    if mutant == 'var767':
        var = (d * d).sum(-1, keepdim=True) / 767.0
    elif mutant == 'uncentred':
        var = (x * x).mean(-1, keepdim=True)
    else:
        var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + (0.0 if mutant == 'noeps' else eps))
    xhat = d * rstd
    d_mean = C_MEAN * E * x.abs().mean(-1, keepdim=True)
    rr = torch.clamp(0.5 * d_mean ** 2 / (var + eps), max=1.0) + 0.5 * (C_VAR * E * var + TINY) / (var + eps) + (1 + 2 * LIBM) * E
    d_xhat = rstd * d_mean + xhat.abs() * (2 * E + rr)
    if dx_in is not None:
        d_xhat = d_xhat + rstd * (dx_in + dx_in.mean(-1, keepdim=True) + xhat.abs() * (xhat.abs() * dx_in).mean(-1, keepdim=True))
    return dict(mean=mean, var=var, rstd=rstd, xhat=xhat, rr=rr, d_xhat=d_xhat)


def ln_fwd(x, gamma, beta, eps, mutant=None, dx_in=None):
    """y = xhat gamma + beta and b_y = |gamma| d_xhat + E |xhat gamma| + E |y| (the two roundings of the affine part)."""
    st = ln_stats(x, eps, mutant, dx_in)
    g, b = gamma.double(), beta.double()
    y = st['xhat'] * g + b
    b_y = g.abs() * st['d_xhat'] + E * (st['xhat'] * g).abs() + E * y.abs()
    return dict(y=y, b_y=b_y)


def sum_slabs_f32(parts, bias, res=None):
    """The pre-LayerNorm sum of sum_layernorm768_kernel in its own fp32 order: bias, then each group of four slabs as
    (t0 + t1) + (t2 + t3), then the tail slabs one by one, then the residual.  Every step is one IEEE fp32 addition."""
    assert parts.dtype == torch.float32 and bias.dtype == torch.float32
    S = parts.shape[0]
    v = bias[None, :].expand(parts.shape[1], D).clone()
    s = 0
    while s + 4 <= S:
        v = v + ((parts[s] + parts[s + 1]) + (parts[s + 2] + parts[s + 3]))
        s += 4
    while s < S:
        v = v + parts[s]
        s += 1
    if res is not None:
        v = v + res
    return v


GELU_ABS = 7e-7          # |gelu_erf - gelu| as vitcap_amd/csrc/common.h states it for its polynomial


def sum_ln_act(parts, bias, gamma, beta, eps):
    """LayerNorm(gelu(bias + sum_s parts[s])) in fp64.  The LayerNorm's input is off by at most
    1.13 (S + 1) E (|bias| + sum |parts|) (the sum's roundings through |gelu'| <= 1.13) + GELU_ABS + E |gelu|."""
    S = parts.shape[0]
    v = bias.double()[None] + parts.double().sum(0)
    mag = bias.double().abs()[None] + parts.double().abs().sum(0)
    gl = 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    dx_in = 1.13 * (S + 1) * E * mag + GELU_ABS + E * gl.abs()
    return ln_fwd(gl, gamma, beta, eps, dx_in=dx_in)


# =====================================================================================================================
# LayerNorm backward and the cast with column sums
# =====================================================================================================================
def ln_bwd_grid(M, n_cu=DEFAULT_CUS):
    """(workgroups, row stride = total waves, trips of the busiest wave) of ln_bwd_grid in vitcap_amd/csrc/train.hip."""
    wgs = 2 * n_cu
    if wgs * NW > M:
        wgs = (M + NW - 1) // NW
    rpw = wgs * NW
    return wgs, rpw, (M + rpw - 1) // rpw


def atomic_sum(terms, d_terms, preset, M, n_cu):
    """preset + column sums over the rows, with the bound: sum d_terms + (trips + NW + workgroups) E (|preset| + sum |terms|).
    The count is the longest chain an addend passes: a wave's trips, the workgroup's NW partials, one atomic per workgroup (the
    last of them onto the preset); multiplied by the sum of magnitudes it holds for every order of the atomics."""
    wgs, rpw, trips = ln_bwd_grid(M, n_cu)
    n = trips + NW + wgs
    tot = preset.double() + terms.sum(0)
    b = n * E * (preset.double().abs() + terms.abs().sum(0))
    if d_terms is not None:
        b = b + d_terms.sum(0)
    return tot, b


def ln_bwd(x, dy, gamma, eps, dres=None, presets=None, n_cu=DEFAULT_CUS, mutant=None):
    """dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)) + dres;  dgamma = preset + sum dy xhat;  dbeta = preset + sum dy.
    presets: (dgamma0, dbeta0) fp32 (768,) or None for zeros.  Bounds (gd = g dy, s1 = mean gd, s2 = mean gd xhat):
      d_s1 = (C_MEAN + 1) E mean|gd|;  d_s2 = mean(|gd| d_xhat) + (C_MEAN + 3) E mean|gd xhat|
      d_t  = E |gd| + d_s1 + |xhat| d_s2 + |s2| d_xhat + E |xhat s2| + 2 E (|gd| + |s1| + |xhat s2|)       (t = the bracket)
      b_dx = rstd d_t + |rstd t| (rr + E) + E |dx|
      dgamma: each addend off by |dy| d_xhat + E |dy xhat|, then atomic_sum;  dbeta: the addends are exact."""
    M = x.shape[0]
    st = ln_stats(x, eps)
    xhat, rstd, rr, d_xhat = st['xhat'], st['rstd'], st['rr'], st['d_xhat']
    g, dyd = gamma.double(), dy.double()
    gd = g * dyd
    s1 = gd.mean(-1, keepdim=True)
    s2 = (gd * xhat).mean(-1, keepdim=True)
    t = gd - (0.0 if mutant == 'no_s1' else s1) - (0.0 if mutant == 'no_s2' else xhat * s2)
    dx = rstd * t
    if dres is not None and mutant != 'no_dres':
        dx = dx + dres.double()
    d_s1 = (C_MEAN + 1) * E * gd.abs().mean(-1, keepdim=True)
    d_s2 = (gd.abs() * d_xhat).mean(-1, keepdim=True) + (C_MEAN + 3) * E * (gd * xhat).abs().mean(-1, keepdim=True)
    d_t = (E * gd.abs() + d_s1 + xhat.abs() * d_s2 + s2.abs() * d_xhat + E * (xhat * s2).abs()
           + 2 * E * (gd.abs() + s1.abs() + (xhat * s2).abs()))
    b_dx = rstd * d_t + (rstd * t).abs() * (rr + E) + E * dx.abs()
    dg0, db0 = presets if presets is not None else (torch.zeros(D), torch.zeros(D))
    tg, tb = dyd * xhat, dyd.clone()
    d_tg = dyd.abs() * d_xhat + E * tg.abs()
    if mutant == 'first_trip_only':                 # the rows of a wave's second and later trips never reach the sums
        rpw = ln_bwd_grid(M, n_cu)[1]
        tg, tb, d_tg = tg[:rpw], tb[:rpw], d_tg[:rpw]
    dgamma, b_dgamma = atomic_sum(tg, d_tg, dg0, M, n_cu)
    dbeta, b_dbeta = atomic_sum(tb, None, db0, M, n_cu)
    return dict(dx=dx, b_dx=b_dx, dgamma=dgamma, b_dgamma=b_dgamma, dbeta=dbeta, b_dbeta=b_dbeta)


def colsum(values, preset, n_cu=DEFAULT_CUS):
    """preset + column sums of the given (already rounded) values, in fp64, with atomic_sum's bound: the addends are exact."""
    return atomic_sum(values.double(), None, preset, values.shape[0], n_cu)


def ln_bwd_cases(n_cu=DEFAULT_CUS):
    """M of the backward and of the cast: one row, the two sides of a workgroup of 8 waves, the older test's size, and the two sizes
    at which a wave takes a second (one row of it) and a third trip (29 rows of it)."""
    return [1, 7, 8, 9, 1157, 16 * n_cu + 1, 32 * n_cu + 29]


def ln_bwd_inputs(M, dy_f32, planted=False, n_cu=DEFAULT_CUS):
    """x (every row kind), dy, gamma, dres, presets of one backward case.  planted: dy is zero in the rows of every wave's first trip
    and carries the sign of x - mean in the others, so that what those rows add to dgamma grows with their number and not with its
    square root (the sum's bound does, through the rows with mean >> std)."""
    wgs, rpw, trips = ln_bwd_grid(M, n_cu)
    x, kind = ln_rows(M, 4000 + M, first_kind=(-rpw) % 7 if trips > 1 else None)     # the first row of a second trip is an ordinary one
    gamma, _ = ln_params(41)
    dy = _uni((M, D), 4100 + M)
    if planted:
        xd = x.double()
        sign = torch.sign(xd - xd.mean(-1, keepdim=True))
        dy = torch.where(sign == 0, dy, dy.abs() * sign.float())
        dy[:ln_bwd_grid(M, n_cu)[1]] = 0.0
    dy = dy.float() if dy_f32 else dy.to(torch.bfloat16)
    dres = _uni((M, D), 4200 + M).float()
    presets = (_uni((D,), 43, 2.0).float(), _uni((D,), 44, 2.0).float(), _uni((D,), 45, 2.0).float())
    return x, dy, gamma, dres, presets


# =====================================================================================================================
# label-smoothed KL
# =====================================================================================================================
def _f32_exp(t):
    """exp as fp32 arithmetic sees its range: overflow to inf above 88.72 (used by the mutants that drop a stable form)."""
    return torch.exp(t).to(torch.float32).double()


def ls_kl(logits, target, eps, row_weight=None, preset=0.0, mutant=None):
    """Per row: lse = max + log sum exp(x - max);  loss_row = sum_v q_v (log q_v - (x_v - lse)) with q = 1 - eps on the target and
    eps / (V - 1) elsewhere;  loss = preset + sum_rows w loss_row, grad = (exp(x - lse) - q) w, w = 1 / rows or row_weight[row].
    logits (rows, V) fp32.  Returns loss, b_loss (scalars), grad, b_grad (rows, V) -- b_grad includes the bf16 store.
      n1 = ceil(V / 1024) + 6 + 16 (a thread's trips, the wave, the 16 wave partials)
      d_lse = (LIBM + n1) E + E max|x - max| + LIBM E |log tot| + E |lse|
      rel p = d_lse + E |x - lse| + LIBM E;   b_grad = |w| (p rel_p + 5 E q + E |p - q|) + 2 E |grad| + U |grad| + TINY"""
    rows, V = logits.shape
    x = logits.double()
    eps = f32(eps)
    q_on, q_off = 1.0 - eps, eps / (V - 1)
    mx = x.max(-1, keepdim=True).values
    if mutant == 'nomax':
        tot = _f32_exp(x).sum(-1, keepdim=True).to(torch.float32).double()
        lse = torch.log(tot)
    else:
        tot = torch.exp(x - mx).sum(-1, keepdim=True)
        lse = mx + torch.log(tot)
    w = torch.full((rows, 1), 1.0 / rows if mutant != 'nomean' else 1.0, dtype=torch.float64)
    if row_weight is not None and mutant != 'noweight':
        w = row_weight.double().view(rows, 1)
    q = torch.full((rows, V), q_off, dtype=torch.float64)
    q.scatter_(1, target.view(-1, 1), 1.0 if mutant == 'target_no_eps' else q_on)
    p = torch.exp(x - lse)
    grad = (p - q) * w
    n1 = (V + 1023) // 1024 + 6 + 16
    d_lse = (LIBM + n1) * E + E * (x - mx).abs().max(-1, keepdim=True).values + LIBM * E * torch.log(tot).abs() + E * lse.abs()
    rel_p = d_lse + E * (x - lse).abs() + LIBM * E
    b_grad = w.abs() * (p * rel_p + 5 * E * q + E * (p - q).abs()) + 2 * E * grad.abs() + U * grad.abs() + TINY
    # the loss
    xt = x.gather(1, target.view(-1, 1))
    sl = x.sum(-1, keepdim=True)
    qt = torch.full((rows, 1), q_on, dtype=torch.float64)
    ent = qt * torch.log(qt) + (eps * math.log(q_off) if eps > 0 else 0.0)
    A = xt - lse
    Bq = (sl - xt) - (V - 1) * lse
    cross = q_on * A + q_off * Bq
    row_loss = (ent - cross) * w
    d_A = d_lse + E * A.abs()
    d_B = n1 * E * x.abs().sum(-1, keepdim=True) + E * (sl - xt).abs() + (V - 1) * d_lse + E * (V - 1) * lse.abs() + E * Bq.abs()
    d_cross = q_on * d_A + 2 * E * (q_on * A).abs() + q_off * d_B + 6 * E * (q_off * Bq).abs() + E * cross.abs()
    d_ent = E * (q_on * (abs(math.log(q_on)) + 1) + (LIBM + 1) * abs(q_on * math.log(q_on))) + E * ent.abs()
    if eps > 0:
        d_ent = d_ent + eps * (LIBM + 1) * E * (1 + abs(math.log(q_off)))
    d_row = (d_ent + d_cross + E * (ent - cross).abs()) * w.abs() + 2 * E * row_loss.abs()
    loss = preset + float(row_loss.sum())
    b_loss = float(d_row.sum()) + (rows + 1) * E * (abs(preset) + float(row_loss.abs().sum()))
    return dict(loss=loss, b_loss=b_loss, grad=grad, b_grad=b_grad)


# (V, ldl, ldd, rows, eps, logits kind, row_weight kind, with dlogits)
KL_LOGITS = ('normal', 'offset80', 'spike60', 'equal')
KL_CASES = [
    (2, 64, 64, 1, 0.1, 'normal', None, True),
    (2, 64, 128, 5, 0.0, 'spike60', 'mixed', True),
    (63, 64, 64, 5, 0.1, 'normal', None, True),
    (63, 64, 64, 33, 0.0, 'equal', 'mixed', True),
    (1000, 1024, 1088, 5, 0.1, 'offset80', None, True),
    (1024, 1024, 1024, 33, 0.1, 'normal', 'mixed', True),
    (1024, 1024, 1024, 1, 0.0, 'spike60', None, True),
    (1025, 1088, 1152, 5, 0.0, 'normal', 'mixed', True),
    (1025, 1088, 1088, 33, 0.1, 'equal', None, True),
    (30522, 30592, 30592, 5, 0.1, 'normal', None, True),
    (30522, 30592, 30592, 5, 0.1, 'normal', None, False),
    (30522, 30592, 30656, 33, 0.0, 'offset80', 'mixed', True),
    (30522, 30592, 30592, 33, 0.1, 'offset80', None, True),
    (30522, 30592, 30592, 1, 0.1, 'spike60', 'mixed', True),
    (30522, 30592, 30592, 5, 0.0, 'equal', 'mixed', True),
]


def kl_case_id(c):
    return 'V%d-ldl%d-ldd%d-r%d-eps%g-%s-%s-%s' % (c[0], c[1], c[2], c[3], c[4], c[5], c[6] or 'mean', 'grad' if c[7] else 'lossonly')


def kl_inputs(case):
    """logits (rows, V) fp32, targets cycling through column 0, V - 1, the row's argmax and its argmin, row_weight or None
    ('mixed': positive, negative and zero weights, the zero on row 0... wherever rows allow), and the loss preset."""
    V, ldl, ldd, rows, eps, kind, wk, with_grad = case
    x = _randn((rows, V), 500 + V + rows, 3.0)
    if kind == 'offset80':
        x = x + 80.0
    elif kind == 'spike60':
        x[torch.arange(rows), (torch.arange(rows) * 7 + 1) % V] = x.max() + 60.0
    elif kind == 'equal':
        x[:] = 1.25
    x = x.float()
    tk = torch.arange(rows) % 4
    tgt = torch.where(tk == 0, torch.zeros(rows, dtype=torch.long),
                      torch.where(tk == 1, torch.full((rows,), V - 1), torch.where(tk == 2, x.argmax(1), x.argmin(1))))
    w = None
    if wk == 'mixed':
        w = _uni((rows,), 600 + rows, 2.0)
        w[0] = 0.0 if rows > 1 else -0.8
        if rows > 1:
            w[1], w[rows - 1] = 0.7, -1.3
        w = w.float()
    return x, tgt, w, 0.75


# =====================================================================================================================
# focal loss and BCE with logits (sums over B x V with a grid-stride loop of 1024 x 256 threads)
# =====================================================================================================================
LOSS_GRID = 1024 * 256
LOSS_CASES = [(1, 30522, 30592), (3, 30522, 30592), (9, 30522, 30592), (300, 1000, 1024)]     # (B, V, ldl)


def _loss_chain(total):
    """Roundings on the longest chain of one addend: a thread's trips, 6 butterfly steps, the 4 wave partials (2), 1024 atomics."""
    return (total + LOSS_GRID - 1) // LOSS_GRID + 6 + 2 + 1024


def loss_inputs(B, V, planted=False):
    """logits (B, V) fp32: N(0, 4) with +-100, +-20, 0 and 1e-6 planted under both labels; labels 0 / 1 with a few 0.5.
    planted: everything before flat index 262144 is a logit of -40 under label 0."""
    x = _randn((B, V), 700 + B, 4.0)
    y = (torch.rand((B, V), generator=_gen(701 + B)) < 0.01).double()
    special = [100.0, -100.0, 20.0, -20.0, 0.0, 1e-6]
    flat_x, flat_y = x.view(-1), y.view(-1)
    n = flat_x.numel()
    for j, s in enumerate(special):
        for lab in (0.0, 1.0):
            i = (n - 1 - (2 * j + int(lab)) * 131) % n           # from the end: inside the planted variant's live range as well
            flat_x[i], flat_y[i] = s, lab
    flat_y[(torch.arange(5) * 977 + n // 2) % n] = 0.5
    if planted:
        flat_x[:LOSS_GRID], flat_y[:LOSS_GRID] = -40.0, 0.0
    return x.float(), y.float()


def _log_sigmoid_parts(x):
    t = torch.exp(-x.abs())
    l1p = torch.log1p(t)
    return l1p, (LIBM * 2) * E * l1p           # expf then log1pf: t / (1 + t) <= log1p(t), so both stay relative to log1p(t)


def focal(logits, label, alpha, preset=0.0, mutant=None):
    """preset - sum [y == 1] alpha (1 - s) logsigmoid(x) + [y == 0] (1 - alpha) s logsigmoid(-x),  s = sigmoid(x).
      d_s = (2 LIBM + 1) E s (expf, the addition, the division);  d_ls = 2 LIBM E log1p(exp(-|x|)) + E |ls|
      addend a (1 - s) ls: a (d_s |ls| + E |1 - s| |ls| + |1 - s| d_ls) + 2 E |addend| + TINY, likewise the other class
      total: sum of those + _loss_chain E (|preset| + sum |addend|)."""
    x, y = logits.double(), label.double()
    alpha = f32(alpha)
    a1, a0 = (1.0 - alpha, alpha) if mutant == 'alpha_swapped' else (alpha, 1.0 - alpha)
    l1p, d_l1p = _log_sigmoid_parts(x)
    s = 1.0 / (1.0 + torch.exp(-x))
    ls = torch.clamp(x, max=0.0) - l1p
    lsn = torch.clamp(-x, max=0.0) - l1p
    if mutant == 'naive_logsigmoid':                  # log(sigmoid(x)) with fp32's range: -inf once exp(-x) overflows
        s32 = 1.0 / (1.0 + _f32_exp(-x))
        ls, lsn = torch.log(s32), torch.log(1.0 / (1.0 + _f32_exp(x)))
    m1, m0 = (1.0, 1.0) if mutant == 'no_modulation' else (1.0 - s, s)
    t1 = torch.where(y == 1.0, a1 * m1 * ls, torch.zeros_like(x))
    t0 = torch.where(y == 0.0, a0 * m0 * lsn, torch.zeros_like(x))
    term = -(t1 + t0)
    if mutant == 'first_trip_only':
        term = term.flatten()[:LOSS_GRID]
    d_s = (2 * LIBM + 1) * E * s
    d_ls, d_lsn = d_l1p + E * ls.abs(), d_l1p + E * lsn.abs()
    d1 = torch.where(y == 1.0, alpha * (d_s * ls.abs() + E * (1 - s) * ls.abs() + (1 - s) * d_ls) + 2 * E * t1.abs() + TINY,
                     torch.zeros_like(x))
    d0 = torch.where(y == 0.0, (1 - alpha) * (d_s * lsn.abs() + E * s * lsn.abs() + s * d_lsn) + 2 * E * t0.abs() + TINY,
                     torch.zeros_like(x))
    total = preset + float(term.sum())
    b = float((d1 + d0).sum()) + _loss_chain(x.numel()) * E * (abs(preset) + float((t1.abs() + t0.abs()).sum()))
    return dict(loss=total, b_loss=b)


def bce(logits, label, preset=0.0, mutant=None):
    """preset + (1 / (B V)) sum max(x, 0) - x y + log1p(exp(-|x|)).
      addend: E |x y| + 2 LIBM E log1p + 2 E (max(x, 0) + |x y| + log1p);  the scale 1 / (B V) and its product: 3 more roundings
      total: scale sum of those + (_loss_chain + 3) E (|preset| + scale sum |addend parts|)."""
    x, y = logits.double(), label.double()
    B, V = x.shape
    l1p, d_l1p = _log_sigmoid_parts(x)
    if mutant == 'naive_log1p':
        l1p = torch.log(1.0 + _f32_exp(-x))
        term = x * (1.0 - y) + l1p                   # max(x, 0) - x y + log1p(exp(-|x|)) == x (1 - y) + log(1 + exp(-x))
    else:
        term = torch.clamp(x, min=0.0) - x * y + l1p
    mag = torch.clamp(x, min=0.0) + (x * y).abs() + l1p
    d_term = E * (x * y).abs() + d_l1p + 2 * E * mag
    scale = 1.0 / B if mutant == 'mean_over_B' else 1.0 / (B * V)
    if mutant == 'first_trip_only':
        term = term.flatten()[:LOSS_GRID]
    total = preset + scale * float(term.sum())
    b = scale * float(d_term.sum()) + (_loss_chain(x.numel()) + 3) * E * (abs(preset) + scale * float(mag.sum()))
    return dict(loss=total, b_loss=b)


# =====================================================================================================================
# gradient norm
# =====================================================================================================================
SUMSQ_GRID = 2048 * 256 * 4                          # floats per trip of sumsq_partial_kernel
SUMSQ_N = [4, 1020, 4096, SUMSQ_GRID, SUMSQ_GRID + 4, 3 * SUMSQ_GRID + 308]
SUMSQ_KINDS = ('random', 'zero', 'one_1e18', 'second_trip_only')


def sumsq_input(n, kind):
    if kind == 'zero':
        return torch.zeros(n)
    g = _uni((n,), 800 + n % 1000).float()
    if kind == 'one_1e18':
        g = g * 1e-3
        g[(n * 5) // 7] = 1e18
    if kind == 'second_trip_only':
        g[:SUMSQ_GRID] = 0.0
    return g


def sumsq(g, mutant=None):
    """sum g^2, bound (trips + 27) E sum g^2: the squares and the two additions of a float4 (3), a thread's trips, 6 butterfly steps
    and the 4 wave partials (2) in each of the two kernels, the final kernel's 8 partials per thread."""
    n = g.numel()
    x = g.double()
    if mutant == 'first_trip_only':
        x = x[:SUMSQ_GRID]
    tot = float((x * x).sum())
    trips = (n + SUMSQ_GRID - 1) // SUMSQ_GRID
    return dict(sumsq=tot, b_sumsq=(trips + 27) * E * float((g.double() ** 2).sum()))


# =====================================================================================================================
# fused clip + AdamW
# =====================================================================================================================
ADAMW_LR_WD = [(1e-4, 0.05), (1e-5, 0.0), (0.0, 0.05), (1e-4, 0.0), (0.1, 0.5), (1e-3, 0.01)]
ADAMW_STEPS = [1, 2, 3, 1000, 20000]
CHUNK = 1024


def adamw_inputs():
    """p U(-1, 1), g U(-3, 3) with a tenth of the entries at 1e-6 of that (sqrt(v) next to eps) and a few exact zeros."""
    n = len(ADAMW_LR_WD) * CHUNK
    p = _uni((n,), 15).float()
    g = _uni((n,), 16, 3.0)
    small = torch.rand(n, generator=_gen(17)) < 0.1
    g = torch.where(small, g * 1e-6, g)
    g[::97] = 0.0
    return p, g.float()


def adamw(p, g, m, v, lr, wd, gsumsq, clip, lr_scale, step, b1=0.9, b2=0.999, eps=1e-8, mutant=None):
    """One fused step on one chunk (lr, wd scalars), from the fp32 p, g, m, v the device starts from.  Returns dp = p_new - p,
    m, v with b_dp, b_m, b_v.  With lr = 0 the chunk is not owned: nothing moves.
      coef = min(1, clip / (sqrt(gsumsq) + 1e-6)): (2 LIBM + 1) E;  ge = g coef: one more
      m' = m b1 + (1 - b1) ge;  v' = v b2 + (1 - b2) ge ge: the products, the sum, d_ge
      bias corrections on the host: powf at LIBM E of b^step, so 1 - b^step is off by LIBM E b^step / (1 - b^step) relative
      step_size = lr bc2s / bc1, upd = step_size m' / (sqrt(v') + eps), p' = p - upd, then p' -= lr wd p'."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    lr0, wd, clip, lr_scale, b1, b2, eps = f32(lr), f32(wd), f32(clip), f32(lr_scale), f32(b1), f32(b2), f32(eps)
    if lr0 == 0.0:
        z = torch.zeros_like(p)
        return dict(dp=z, b_dp=z, m=m, b_m=z, v=v, b_v=z)
    lr = lr0 * (1.0 if mutant == 'no_lr_scale' else lr_scale)
    norm = math.sqrt(gsumsq)
    coef = clip / (norm + f32(1e-6))
    if mutant == 'no_clip':
        coef = 1.0
    elif mutant != 'always_scale':
        coef = min(coef, 1.0)
    ge = g * coef
    d_ge = (2 * LIBM + 2) * E * ge.abs()
    m2 = m * b1 + (1.0 - b1) * ge
    v2 = v if mutant == 'v_frozen' else v * b2 + (1.0 - b2) * ge * ge
    b_m = E * (m * b1).abs() + (1.0 - b1) * d_ge + E * ((1.0 - b1) * ge).abs() + E * m2.abs()
    b_v = E * (v * b2).abs() + (1.0 - b2) * (2 * ge.abs() * d_ge + 2 * E * ge * ge) + E * v2.abs() + TINY
    P1, P2 = b1 ** step, b2 ** step
    bc1, bc2 = 1.0 - P1, 1.0 - P2
    bc2s = bc2 if mutant == 'bc2_no_sqrt' else math.sqrt(bc2)
    rel_ss = LIBM * E * P1 / bc1 + E + 0.5 * (LIBM * E * P2 / bc2 + E) + LIBM * E + (3 + LIBM) * E
    step_size = lr * bc2s / bc1
    sq = torch.sqrt(v2)
    denom = torch.sqrt(v2 + eps) if mutant == 'eps_inside' else sq + eps
    d_sq = torch.where(sq > 0, 0.5 * b_v / torch.clamp(sq, min=1e-300), torch.sqrt(b_v)) + LIBM * E * sq
    d_den = d_sq + E * denom
    r = m2 / denom
    d_r = b_m / denom + r.abs() * d_den / denom + LIBM * E * r.abs()
    upd = step_size * r
    d_upd = upd.abs() * (rel_ss + E) + abs(step_size) * d_r
    if mutant == 'decay_first':
        pe = (p - lr * wd * p) - upd
        return dict(dp=pe - p, m=m2, v=v2)
    pe = p - upd
    b_dp = d_upd + E * pe.abs()
    if wd > 0.0 and mutant != 'no_decay':
        pe2 = pe - lr * wd * pe
        b_dp = b_dp * (1.0 + lr * wd) + 3 * E * (lr * wd * pe).abs() + E * pe2.abs()
        pe = pe2
    return dict(dp=pe - p, b_dp=b_dp, m=m2, b_m=b_m, v=v2, b_v=b_v)
