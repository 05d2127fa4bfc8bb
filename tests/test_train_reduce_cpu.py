"""Teeth of tests/test_hip_train_reduce.py, checked without a GPU and without a kernel (docs/LAB_tests_train_reduce.md).

The GPU file compares each kernel with its fp64 reference (oracle/train_reduce_ref.py) element by element under derived bounds.  A
kernel that carries an error sits within one bound of the equally wrong reference, so it is certain to fail only where the wrong and
the right reference are more than two bounds apart.  This file requires that distance (KILL = 2), for every mutant of every
reference, on the GPU file's own inputs: a condition on the inputs, never on the bounds.  It also runs plain fp32 arithmetic (torch
on the CPU, in torch's own summation order) against every bound: a term missing from a derivation shows here, before a GPU run.
"""
import math

import pytest
import torch

from oracle import train_reduce_ref as R

KILL = 2.0
CUS = R.DEFAULT_CUS


def _ratio(wrong, right, bound):
    """Largest |wrong - right| / bound; a NaN or an infinity in `wrong`, or a move where the bound is zero, counts as infinite."""
    wrong = torch.as_tensor(wrong, dtype=torch.float64)
    right = torch.as_tensor(right, dtype=torch.float64)
    bound = torch.as_tensor(bound, dtype=torch.float64)
    d = (wrong - right).abs()
    r = torch.where(d > 0, d / bound, torch.zeros_like(d))
    r = torch.where(torch.isfinite(wrong), r, torch.full_like(r, float('inf')))
    return float(torch.nan_to_num(r, nan=float('inf'), posinf=float('inf')).max())


def _killed(name, ratios):
    """ratios: {case: distance in bounds}.  The mutant must be KILL bounds away on at least one case; prints the case that does it."""
    case = max(ratios, key=ratios.get)
    print('TEETH %-28s killed by %-40s at %.3g bounds' % (name, case, ratios[case]))
    assert ratios[case] > KILL, '%s stays within %.1f bounds on every case: %s' % (name, KILL, ratios)


def _inside(name, got, ref, bound):
    r = _ratio(got, ref, bound)
    print('ROOM  %-40s fp32 arithmetic at %.3f bounds' % (name, r))
    assert r <= 1.0, '%s: plain fp32 arithmetic is %.3g bounds from the reference' % (name, r)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm forward
# ---------------------------------------------------------------------------------------------------------------------
LN_FWD = [(M, eps) for M in (1, 3, 4, 5, 1157) for eps in (1e-6, 1e-12)]


@pytest.mark.parametrize('mutant', ['var767', 'noeps', 'uncentred'])
def test_layernorm_forward_mutants(mutant):
    gamma, beta = R.ln_params(40)
    ratios = {}
    for M, eps in LN_FWD:
        x, _ = R.ln_rows(M, 3000 + M)
        right = R.ln_fwd(x, gamma, beta, eps)
        wrong = R.ln_fwd(x, gamma, beta, eps, mutant=mutant)
        ratios['M%d-eps%g' % (M, eps)] = _ratio(wrong['y'], right['y'], right['b_y'])
    _killed('ln_fwd ' + mutant, ratios)


def _ln_fwd_f32(x, gamma, beta, eps):
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    return d * rstd * gamma + beta


@pytest.mark.parametrize('M,eps', LN_FWD)
def test_layernorm_forward_bound_has_room(M, eps):
    gamma, beta = R.ln_params(40)
    x, kind = R.ln_rows(M, 3000 + M)
    ref = R.ln_fwd(x, gamma, beta, eps)
    assert bool(torch.isfinite(ref['b_y']).all())
    _inside('ln_fwd M%d eps%g' % (M, eps), _ln_fwd_f32(x, gamma, beta, eps), ref['y'], ref['b_y'])
    zero = (kind == R.LN_KINDS.index('zero'))
    if zero.any():                                            # a zero row: beta exactly, and nothing in the bound but E |beta|
        assert torch.equal(ref['y'][zero], beta.double().expand(int(zero.sum()), R.D))
        assert bool((ref['b_y'][zero] <= R.E * beta.double().abs()).all())
    ordinary = (kind == R.LN_KINDS.index('ordinary'))
    const = (kind == R.LN_KINDS.index('constant'))
    if eps == 1e-12 and ordinary.any() and const.any():      # the same formula: tight on an ordinary row, wide on a constant one
        assert float(ref['b_y'][ordinary].max()) < 1e-5 and float(ref['b_y'][const].max()) > 0.1


def test_slab_sum_emulation_order():
    """sum_slabs_f32 is the kernel's order: bias first, groups of four as (t0 + t1) + (t2 + t3), the tail one by one, the residual last.
    Shown on values where every other order gives other bits."""
    big, one = 2.0 ** 24, 1.0
    f = lambda *v: torch.tensor(v, dtype=torch.float32).view(-1, 1, 1).expand(-1, 1, R.D).contiguous()
    bias = torch.zeros(R.D)
    # (big + 1) + (1 + 1): big + 1 rounds to big (even), 1 + 1 = 2 survives: big + 2
    assert float(R.sum_slabs_f32(f(big, one, one, one), bias)[0, 0]) == big + 2
    # five slabs: the fifth is added on its own: (big + 2) + 1 is a tie and goes to the even neighbour big + 4 (one by one: big)
    assert float(R.sum_slabs_f32(f(big, one, one, one, one), bias)[0, 0]) == big + 4
    # three slabs: no group of four, one by one from the bias: ((0 + big) + 1) + 1 = big
    assert float(R.sum_slabs_f32(f(big, one, one), bias)[0, 0]) == big
    # the residual comes last: (bias + slab) + res
    assert float(R.sum_slabs_f32(f(one), torch.full((R.D,), big), torch.full((1, R.D), one))[0, 0]) == big
    assert float(R.sum_slabs_f32(f(-big), torch.full((R.D,), big), torch.full((1, R.D), one))[0, 0]) == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def bwd_refs():
    """Right references of the backward cases the mutants are tried on (dy bf16; the planted variant at the first looping size)."""
    out = {}
    for M, planted in [(7, False), (9, False), (1157, False), (16 * CUS + 1, False), (16 * CUS + 1, True), (32 * CUS + 29, True)]:
        x, dy, gamma, dres, presets = R.ln_bwd_inputs(M, False, planted, CUS)
        out[(M, planted)] = (x, dy, gamma, dres, presets, R.ln_bwd(x, dy, gamma, 1e-6, dres, presets[:2], CUS))
    return out


@pytest.mark.parametrize('mutant', ['no_s1', 'no_s2', 'no_dres', 'first_trip_only'])
def test_layernorm_backward_mutants(bwd_refs, mutant):
    ratios = {}
    for (M, planted), (x, dy, gamma, dres, presets, right) in bwd_refs.items():
        wrong = R.ln_bwd(x, dy, gamma, 1e-6, dres, presets[:2], CUS, mutant=mutant)
        name = 'M%d%s' % (M, '-planted' if planted else '')
        if mutant == 'first_trip_only':
            ratios[name] = min(_ratio(wrong['dgamma'], right['dgamma'], right['b_dgamma']),
                               _ratio(wrong['dbeta'], right['dbeta'], right['b_dbeta']))
        else:
            ratios[name] = _ratio(wrong['dx'], right['dx'], right['b_dx'])
    _killed('ln_bwd ' + mutant, ratios)
    if mutant == 'first_trip_only':        # every planted case shows it, in both sums; where no wave loops there is nothing to show
        for name, r in ratios.items():
            assert r > KILL if 'planted' in name else (r == 0.0 or name == 'M%d' % (16 * CUS + 1)), (name, r)


def test_layernorm_backward_colsum_of_unrounded_dx(bwd_refs):
    ratios = {}
    for (M, planted), (x, dy, gamma, dres, presets, right) in bwd_refs.items():
        dxf = right['dx'].float()
        want, b = R.colsum(R.rne_bf16(dxf), presets[2], CUS)
        wrong, _ = R.colsum(dxf, presets[2], CUS)
        ratios['M%d%s' % (M, '-planted' if planted else '')] = _ratio(wrong, want, b)
    _killed('ln_bwd colsum unrounded', ratios)


@pytest.mark.parametrize('M', [7, 1157])
def test_layernorm_backward_bound_has_room(M):
    x, dy, gamma, dres, presets = R.ln_bwd_inputs(M, True, False, CUS)
    ref = R.ln_bwd(x, dy, gamma, 1e-6, dres, presets[:2], CUS)
    for n in ('b_dx', 'b_dgamma', 'b_dbeta'):
        assert bool(torch.isfinite(ref[n]).all()), n
    xx = x.clone().requires_grad_(True)
    gg = gamma.clone().requires_grad_(True)
    bb = torch.zeros(R.D, requires_grad=True)
    torch.nn.functional.layer_norm(xx, (R.D,), gg, bb, 1e-6).backward(dy)
    _inside('ln_bwd dx M%d' % M, xx.grad + dres, ref['dx'], ref['b_dx'])
    _inside('ln_bwd dgamma M%d' % M, presets[0] + gg.grad, ref['dgamma'], ref['b_dgamma'])
    _inside('ln_bwd dbeta M%d' % M, presets[1] + bb.grad, ref['dbeta'], ref['b_dbeta'])


def test_backward_grid_is_the_launchers():
    """ln_bwd_grid of train.hip: 2 workgroups of 8 waves per CU, fewer when M is smaller; the stride is the total number of waves."""
    assert R.ln_bwd_grid(1, 256) == (1, 8, 1) and R.ln_bwd_grid(9, 256) == (2, 16, 1) and R.ln_bwd_grid(1157, 256) == (145, 1160, 1)
    assert R.ln_bwd_grid(4096, 256) == (512, 4096, 1) and R.ln_bwd_grid(4097, 256) == (512, 4096, 2)
    assert R.ln_bwd_grid(32 * 256 + 29, 256) == (512, 4096, 3) and R.ln_bwd_grid(16 * 304 + 1, 304) == (608, 4864, 2)


# ---------------------------------------------------------------------------------------------------------------------
# label-smoothed KL
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def kl_refs():
    out = {}
    for case in R.KL_CASES:
        if not case[7] or (case[0] == 30522 and case[3] == 33 and case[5] != 'offset80'):
            continue
        x, tgt, w, preset = R.kl_inputs(case)
        out[case] = (x, tgt, w, preset, R.ls_kl(x, tgt, case[4], w, preset))
    return out


@pytest.mark.parametrize('mutant', ['target_no_eps', 'noweight', 'nomean', 'nomax'])
def test_ls_kl_mutants(kl_refs, mutant):
    grad, loss = {}, {}
    for case, (x, tgt, w, preset, right) in kl_refs.items():
        wrong = R.ls_kl(x, tgt, case[4], w, preset, mutant=mutant)
        grad[R.kl_case_id(case)] = _ratio(wrong['grad'], right['grad'], right['b_grad'])
        loss[R.kl_case_id(case)] = _ratio(wrong['loss'], right['loss'], right['b_loss'])
    _killed('ls_kl grad ' + mutant, grad)
    if mutant != 'target_no_eps':                     # that one is an error of the gradient alone
        _killed('ls_kl loss ' + mutant, loss)
    if mutant == 'nomax':
        off = [k for k in loss if 'offset80' in k and 'V30522' in k]
        # exp(80 + 3 * 4.2) overflows fp32: the row sum and the loss are inf, and exp(x - inf) = 0 leaves -q w as the whole gradient
        assert off and all(math.isinf(loss[k]) and grad[k] > KILL for k in off), 'the offset case must overflow without the max'


def _ls_kl_f32(x, tgt, eps, w, preset):
    """The kernel's statements in torch fp32 (torch's own order inside each sum)."""
    rows, V = x.shape
    t = lambda s: torch.tensor(s, dtype=torch.float32)
    mx = x.max(1, keepdim=True).values
    lse = mx + torch.log(torch.exp(x - mx).sum(1, keepdim=True))
    q_on, q_off = t(1.0) - t(eps), t(eps) / t(float(V - 1))
    wt = (w if w is not None else (t(1.0) / t(float(rows))).expand(rows)).view(rows, 1)
    q = q_off.expand(rows, V).clone().scatter(1, tgt.view(-1, 1), q_on.expand(rows, 1))
    grad = (torch.exp(x - lse) - q) * wt
    xt = x.gather(1, tgt.view(-1, 1))
    ent = q_on * torch.log(q_on) + (t(eps) * torch.log(q_off) if eps > 0 else t(0.0))
    cross = q_on * (xt - lse) + q_off * ((x.sum(1, keepdim=True) - xt) - t(float(V - 1)) * lse)
    loss = t(preset)
    for r in range(rows):
        loss = loss + ((ent - cross) * wt)[r, 0]
    return float(loss), grad.to(torch.bfloat16).double()


def test_ls_kl_bound_has_room(kl_refs):
    for case, (x, tgt, w, preset, ref) in kl_refs.items():
        assert bool(torch.isfinite(ref['b_grad']).all()) and math.isfinite(ref['b_loss'])
        loss, grad = _ls_kl_f32(x, tgt, case[4], w, preset)
        _inside('ls_kl grad ' + R.kl_case_id(case), grad, ref['grad'], ref['b_grad'])
        _inside('ls_kl loss ' + R.kl_case_id(case), loss, ref['loss'], ref['b_loss'])
        if w is not None and float(w[0]) == 0.0:
            assert float(ref['grad'][0].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# focal, BCE
# ---------------------------------------------------------------------------------------------------------------------
def _loss_variants():
    for B, V, ldl in R.LOSS_CASES:
        yield 'B%d-V%d' % (B, V), R.loss_inputs(B, V)
        if B * V > R.LOSS_GRID:
            yield 'B%d-V%d-planted' % (B, V), R.loss_inputs(B, V, planted=True)


@pytest.fixture(scope='module')
def loss_inputs():
    return dict(_loss_variants())


@pytest.mark.parametrize('mutant', ['alpha_swapped', 'no_modulation', 'naive_logsigmoid', 'first_trip_only'])
def test_focal_mutants(loss_inputs, mutant):
    ratios = {}
    for name, (x, y) in loss_inputs.items():
        for alpha in (0.5, 0.25):
            right = R.focal(x, y, alpha, 1.5)
            wrong = R.focal(x, y, alpha, 1.5, mutant=mutant)
            ratios['%s-a%g' % (name, alpha)] = _ratio(wrong['loss'], right['loss'], right['b_loss'])
    _killed('focal ' + mutant, ratios)
    if mutant == 'first_trip_only':
        assert all(r > KILL for k, r in ratios.items() if 'planted' in k), ratios


@pytest.mark.parametrize('mutant', ['mean_over_B', 'naive_log1p', 'first_trip_only'])
def test_bce_mutants(loss_inputs, mutant):
    ratios = {}
    for name, (x, y) in loss_inputs.items():
        right = R.bce(x, y, -0.5)
        ratios[name] = _ratio(R.bce(x, y, -0.5, mutant=mutant)['loss'], right['loss'], right['b_loss'])
    _killed('bce ' + mutant, ratios)
    if mutant == 'first_trip_only':
        assert all(r > KILL for k, r in ratios.items() if 'planted' in k), ratios


def test_focal_bce_bounds_have_room(loss_inputs):
    for name, (x, y) in loss_inputs.items():
        s = torch.sigmoid(x)
        f = -(torch.where(y == 1, 0.25 * (1 - s) * torch.nn.functional.logsigmoid(x), torch.zeros_like(x))
              + torch.where(y == 0, 0.75 * s * torch.nn.functional.logsigmoid(-x), torch.zeros_like(x))).sum()
        ref = R.focal(x, y, 0.25, 1.5)
        _inside('focal ' + name, float(f) + 1.5, ref['loss'], ref['b_loss'])
        b = torch.nn.functional.binary_cross_entropy_with_logits(x, y)
        ref = R.bce(x, y, -0.5)
        _inside('bce ' + name, float(b) - 0.5, ref['loss'], ref['b_loss'])
        half = R.focal(x, torch.where(y == 0.5, torch.full_like(y, 0.3), y), 0.25, 1.5)
        assert half['loss'] == R.focal(x, y, 0.25, 1.5)['loss'], 'a label that is neither 0 nor 1 contributes nothing'


# ---------------------------------------------------------------------------------------------------------------------
# gradient norm
# ---------------------------------------------------------------------------------------------------------------------
def test_sumsq_mutant_and_room():
    ratios = {}
    for n in R.SUMSQ_N:
        for kind in R.SUMSQ_KINDS:
            if kind == 'second_trip_only' and n <= R.SUMSQ_GRID:
                continue
            g = R.sumsq_input(n, kind)
            right = R.sumsq(g)
            ratios['n%d-%s' % (n, kind)] = _ratio(R.sumsq(g, mutant='first_trip_only')['sumsq'], right['sumsq'], right['b_sumsq'])
            _inside('sumsq n%d %s' % (n, kind), float((g * g).sum()), right['sumsq'], right['b_sumsq'])
    _killed('sumsq first_trip_only', ratios)
    assert all(r > KILL for k, r in ratios.items() if 'second_trip_only' in k), ratios


# ---------------------------------------------------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------------------------------------------------
ADAMW_SETTINGS = [   # (name, clip, lr_scale): the gradient norm of adamw_inputs() is about 128
    ('clipped', 1.0, 1.0), ('unclipped', 1e4, 1.0), ('clipped-scale0.37', 1.0, 0.37),
]


def _adamw_f32(p, g, m, v, lr, wd, gsumsq, clip, lr_scale, step, b1=0.9, b2=0.999, eps=1e-8):
    """The kernel's statements in torch fp32."""
    t = lambda s: torch.tensor(s, dtype=torch.float32)
    coef = torch.minimum(t(clip) / (torch.sqrt(t(gsumsq)) + t(1e-6)), t(1.0))
    lr_ = t(lr) * t(lr_scale)
    bc1 = t(1.0) - torch.pow(t(b1), t(float(step)))
    bc2s = torch.sqrt(t(1.0) - torch.pow(t(b2), t(float(step))))
    ss = lr_ * bc2s / bc1
    ge = g * coef
    m2 = m * t(b1) + (t(1.0) - t(b1)) * ge
    v2 = v * t(b2) + (t(1.0) - t(b2)) * ge * ge
    pe = p - ss * (m2 / (torch.sqrt(v2) + t(eps)))
    if wd > 0:
        pe = pe - lr_ * t(wd) * pe
    return pe, m2, v2


@pytest.fixture(scope='module')
def adamw_runs():
    """For each setting: the state before each step of R.ADAMW_STEPS (carried by the fp32 emulation) and the right reference."""
    p0, g = R.adamw_inputs()
    gsumsq = float((g.double() ** 2).sum().float())
    runs = []
    for name, clip, lr_scale in ADAMW_SETTINGS:
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        for step in R.ADAMW_STEPS:
            new = [t.clone() for t in (p, m, v)]
            for c, (lr, wd) in enumerate(R.ADAMW_LR_WD):
                sl = slice(c * R.CHUNK, (c + 1) * R.CHUNK)
                if lr == 0.0:
                    continue
                new[0][sl], new[1][sl], new[2][sl] = _adamw_f32(p[sl], g[sl], m[sl], v[sl], lr, wd, gsumsq, clip, lr_scale, step)
            runs.append((name, clip, lr_scale, step, (p, m, v), tuple(new), g, gsumsq))
            p, m, v = new
    return runs


ADAMW_MUTANTS = ['no_decay', 'decay_first', 'bc2_no_sqrt', 'eps_inside', 'no_clip', 'always_scale', 'v_frozen', 'no_lr_scale']


@pytest.mark.parametrize('mutant', ADAMW_MUTANTS)
def test_adamw_mutants(adamw_runs, mutant):
    ratios = {}
    for name, clip, lr_scale, step, (p, m, v), new, g, gsumsq in adamw_runs:
        for c, (lr, wd) in enumerate(R.ADAMW_LR_WD):
            if lr == 0.0:
                continue
            sl = slice(c * R.CHUNK, (c + 1) * R.CHUNK)
            a = (p[sl], g[sl], m[sl], v[sl], lr, wd, gsumsq, clip, lr_scale, step)
            right, wrong = R.adamw(*a), R.adamw(*a, mutant=mutant)
            ratios['%s-step%d-lr%g-wd%g' % (name, step, lr, wd)] = max(
                _ratio(wrong[n], right[n], right['b_' + n]) for n in ('dp', 'm', 'v'))
    _killed('adamw ' + mutant, ratios)
    if mutant == 'decay_first':
        assert ratios['clipped-step1-lr0.1-wd0.5'] > KILL, 'the planted chunk is there for this one'


def test_adamw_bound_has_room(adamw_runs):
    for name, clip, lr_scale, step, (p, m, v), new, g, gsumsq in adamw_runs:
        for c, (lr, wd) in enumerate(R.ADAMW_LR_WD):
            sl = slice(c * R.CHUNK, (c + 1) * R.CHUNK)
            ref = R.adamw(p[sl], g[sl], m[sl], v[sl], lr, wd, gsumsq, clip, lr_scale, step)
            tag = 'adamw %s step%d lr%g wd%g ' % (name, step, lr, wd)
            _inside(tag + 'dp', new[0][sl].double() - p[sl].double(), ref['dp'], ref['b_dp'])
            _inside(tag + 'm', new[1][sl], ref['m'], ref['b_m'])
            _inside(tag + 'v', new[2][sl], ref['v'], ref['b_v'])
