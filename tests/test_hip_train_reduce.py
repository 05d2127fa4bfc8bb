"""Per-element parity of the kernels that close the training step -- LayerNorm forward / split-K LayerNorm / LayerNorm backward, the
bf16 cast with column sums, the three losses, the gradient norm, the fused clip + AdamW -- with the fp64 references of
oracle/train_reduce_ref.py at loop and range edges (docs/LAB_tests_train_reduce.md).

Every comparison is |got - ref| <= bound per element, the bound derived from the kernel's rounding points; no aggregate norm and no
element left out.  Outputs are pre-filled with the sentinel (fp32 0x7B7B7B7B, bf16 0x7B7B) and followed by guard rows or elements
that must still hold it afterwards; the padding of the inputs (columns 768..ld, slab gaps, rows behind M) holds NaN, so a read of
it shows.  tests/test_train_reduce_cpu.py proves without a GPU that every mutant of a reference is more than two bounds from the
right one on these inputs.  Each comparison prints its largest error / bound, and the module prints the maxima at the end (`-s`).
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from oracle import train_reduce_ref as R

pytestmark = pytest.mark.gpu

SENT16 = 0x7B7B
SENT32 = 0x7B7B7B7B
D = R.D
MAXIMA = {}


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vitcap_amd import ops as o
    return o


@pytest.fixture(scope='module')
def lib(ops):
    from vitcap_amd._lib import lib as l
    return l


@pytest.fixture(scope='module')
def n_cu(ops):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for k in sorted(MAXIMA):
        print('MAXIMUM %-28s err/bound %.3f  (%s)' % ((k,) + MAXIMA[k]))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sent_f32(*shape):
    return torch.full(shape, SENT32, dtype=torch.int32, device='cuda').view(torch.float32)


def _sent_bf16(*shape):
    return torch.full(shape, SENT16, dtype=torch.int16, device='cuda').view(torch.bfloat16)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _all_sent(t):
    b = _bits(t)
    return bool((b == (SENT16 if b.dtype == torch.int16 else SENT32)).all())


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _nan_padded(t, rows, ld):
    """(M, 768) fp32 -> device (rows, ld) with NaN wherever the kernel may not read; returns the buffer."""
    buf = torch.full((rows, ld), float('nan'), dtype=t.dtype)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf.cuda()


def _within(key, what, got, want, bound):
    """|got - want| <= bound at every element (a NaN or a left-over sentinel is off); keeps the largest err / bound per key."""
    got = torch.as_tensor(got, dtype=torch.float64).cpu()
    want = torch.as_tensor(want, dtype=torch.float64)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs()
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float('inf')), ratio).reshape(-1)
    i = int(ratio.argmax()) if ratio.numel() else 0
    top = float(ratio[i]) if ratio.numel() else 0.0
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(want.shape))) if want.dim() else ()
    print('MEASURED %s %s: largest err/bound %.3f at %s (err %.3e, bound %.3e, want %.3e)' % (
        key, what, top, idx, float(err.reshape(-1)[i]), float(bound.reshape(-1)[i]), float(want.reshape(-1)[i])))
    if key not in MAXIMA or top > MAXIMA[key][0]:
        MAXIMA[key] = (top, what)
    bad = ~(err <= bound)
    assert not bad.any(), '%s %s: %d/%d elements beyond their bound, largest err/bound %.3g at %s' % (
        key, what, int(bad.sum()), bad.numel(), top, idx)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm forward
# ---------------------------------------------------------------------------------------------------------------------
def _ln_fwd(lib, xbuf, ldx, gamma, beta, eps, M, want_b=True, want_f=True):
    """One call on sentinel outputs with one guard row; returns (yb, yf) of M + 1 rows on the device (None where not asked for)."""
    yb = _sent_bf16(M + 1, D) if want_b else None
    yf = _sent_f32(M + 1, D) if want_f else None
    rc = lib.vitcap_layernorm_fwd(_p(xbuf), ldx, _p(gamma), _p(beta), eps, _p(yb), _p(yf), M, D, _s())
    assert rc == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    for t in (yb, yf):
        assert t is None or _all_sent(t[M:]), 'the guard row was written'
    return yb, yf


@pytest.mark.parametrize('eps', [1e-6, 1e-12])
@pytest.mark.parametrize('ldx', [768, 832])
@pytest.mark.parametrize('M', [1, 3, 4, 5, 1157])
def test_layernorm_forward(lib, ops, M, ldx, eps):
    x, kind = R.ln_rows(M, 3000 + M)
    gamma, beta = R.ln_params(40)
    ref = R.ln_fwd(x, gamma, beta, eps)
    xbuf, g, b = _nan_padded(x, M + 2, ldx), gamma.cuda(), beta.cuda()
    yb, yf = _ln_fwd(lib, xbuf, ldx, g, b, eps, M)
    what = 'M%d-ldx%d-eps%g' % (M, ldx, eps)
    _within('layernorm y', what, yf[:M], ref['y'], ref['b_y'])
    assert torch.equal(yb[:M].cpu(), yf[:M].cpu().to(torch.bfloat16)), 'yb is not RNE(yf)'
    zero = kind == R.LN_KINDS.index('zero')
    assert _same_bits(yf[:M][zero.cuda()], beta.expand(int(zero.sum()), D)), 'a zero row must give beta bit for bit'
    only_b, _ = _ln_fwd(lib, xbuf, ldx, g, b, eps, M, want_f=False)
    _, only_f = _ln_fwd(lib, xbuf, ldx, g, b, eps, M, want_b=False)
    assert _same_bits(only_b, yb) and _same_bits(only_f, yf)
    if ldx == 768:
        ob, of = ops.layernorm(xbuf[:M], g, b, eps, want_bf16=True, want_f32=True)
        assert _same_bits(ob, yb[:M]) and _same_bits(of, yf[:M])


# ---------------------------------------------------------------------------------------------------------------------
# split-K LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def _slabs(S, M, seed):
    """S slabs of (M, 768) fp32 whose magnitudes spread over four decades (the order of the additions shows in the bits), laid out
    with a gap of 256 NaN floats behind each slab: (device buffer, stride, the slabs on the CPU)."""
    parts = R._randn((S, M, D), seed) * (10.0 ** torch.randint(-2, 3, (S, M, D), generator=torch.Generator().manual_seed(seed + 1)))
    parts = parts.float()
    stride = M * D + 256
    buf = torch.full((S, stride), float('nan'))
    buf[:, :M * D] = parts.view(S, M * D)
    return buf.cuda(), stride, parts.contiguous()


def _sum_ln(lib, buf, S, stride, bias, res, ldr, act, gamma, beta, eps, M):
    yb, yf = _sent_bf16(M + 1, D), _sent_f32(M + 1, D)
    rc = lib.vitcap_sum_layernorm(_p(buf), S, stride, _p(bias), _p(res), ldr, act, _p(gamma), _p(beta), eps, _p(yb), _p(yf), M, D, _s())
    assert rc == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    assert _all_sent(yb[M:]) and _all_sent(yf[M:]), 'the guard row was written'
    return yb, yf


@pytest.mark.parametrize('M', [1, 64, 130])
@pytest.mark.parametrize('S', [1, 2, 3, 4, 5, 8, 9])
def test_sum_layernorm_is_layernorm_of_the_emulated_sum(lib, ops, S, M):
    """Without the activation the kernel is ln_row on bias + slabs + residual added in a fixed fp32 order: vitcap_layernorm_fwd on
    that sum, emulated addition by addition, gives the same bits (ln_row is the one copy), and the sum's LayerNorm meets its bound."""
    buf, stride, parts = _slabs(S, M, 5000 + 10 * S + M)
    gamma, beta = R.ln_params(46)
    bias = R._uni((D,), 47).float()
    res = R._randn((M, D), 48 + M, 2.0).float()
    g, b = gamma.cuda(), beta.cuda()
    for with_res in (True, False):
        rbuf = _nan_padded(res, M + 1, 832) if with_res else None
        yb, yf = _sum_ln(lib, buf, S, stride, bias.cuda(), rbuf, 832 if with_res else 0, 0, g, b, 1e-12, M)
        v = R.sum_slabs_f32(parts, bias, res if with_res else None)
        wb, wf = _ln_fwd(lib, v.cuda(), D, g, b, 1e-12, M)
        assert _same_bits(yf, wf) and _same_bits(yb, wb), 'S=%d M=%d residual=%s' % (S, M, with_res)
        ref = R.ln_fwd(v, gamma, beta, 1e-12)
        _within('sum_layernorm y', 'S%d-M%d-res%d' % (S, M, with_res), yf[:M], ref['y'], ref['b_y'])
    if S == 5:                                  # the wrapper passes the tensor's own slab stride
        ob, of = ops.sum_layernorm(parts.cuda(), bias.cuda(), None, g, b, 1e-12)
        assert _same_bits(ob, yb[:M]) and _same_bits(of, yf[:M])


@pytest.mark.parametrize('S,M', [(3, 130), (8, 64), (9, 1)])
def test_sum_layernorm_with_activation(lib, S, M):
    buf, stride, parts = _slabs(S, M, 5500 + S)
    gamma, beta = R.ln_params(46)
    bias = R._uni((D,), 47).float()
    yb, yf = _sum_ln(lib, buf, S, stride, bias.cuda(), None, 0, 1, gamma.cuda(), beta.cuda(), 1e-6, M)
    ref = R.sum_ln_act(parts, bias, gamma, beta, 1e-6)
    _within('sum_layernorm+gelu y', 'S%d-M%d' % (S, M), yf[:M], ref['y'], ref['b_y'])
    assert torch.equal(yb[:M].cpu(), yf[:M].cpu().to(torch.bfloat16))


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 16               # sentinel floats behind each 768-wide accumulator


def _acc(preset):
    """A 768-wide accumulator holding `preset`, followed by GUARD sentinel floats."""
    t = _sent_f32(D + GUARD)
    t[:D] = preset.cuda()
    return t


def _ln_bwd(lib, xbuf, ldx, dyb, gamma, eps, dres, M, presets, want_f=True, want_b=True, colsum=True):
    dxf = _sent_f32(M + 1, D) if want_f else None
    dxb = _sent_bf16(M + 1, D) if want_b else None
    dg, db = _acc(presets[0]), _acc(presets[1])
    cs = _acc(presets[2]) if colsum else None
    rc = lib.vitcap_layernorm_bwd(_p(xbuf), ldx, _p(dyb), int(dyb.dtype == torch.float32), _p(gamma), eps, _p(dres), _p(dxf), _p(dxb),
                                  _p(dg), _p(db), _p(cs), M, D, _s())
    assert rc == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    for t in (dxf, dxb):
        assert t is None or _all_sent(t[M:]), 'the guard row of dx was written'
    for t in (dg, db, cs):
        assert t is None or _all_sent(t[D:]), 'the guard behind an accumulator was written'
    return dxf, dxb, dg, db, cs


def _check_ln_bwd(lib, n_cu, M, dy_f32, with_res, planted):
    x, dy, gamma, dres, presets = R.ln_bwd_inputs(M, dy_f32, planted, n_cu)
    ldx = 832 if with_res else 768
    xbuf, dyb = _nan_padded(x, M + 1, ldx), _nan_padded(dy, M + 1, D)
    drb = _nan_padded(dres, M + 1, D) if with_res else None
    ref = R.ln_bwd(x, dy, gamma, 1e-6, dres if with_res else None, presets[:2], n_cu)
    dxf, dxb, dg, db, cs = _ln_bwd(lib, xbuf, ldx, dyb, gamma.cuda(), 1e-6, drb, M, presets)
    what = 'M%d-%s-res%d%s' % (M, 'f32' if dy_f32 else 'bf16', with_res, '-planted' if planted else '')
    _within('layernorm_bwd dx', what, dxf[:M], ref['dx'], ref['b_dx'])
    _within('layernorm_bwd dgamma', what, dg[:D], ref['dgamma'], ref['b_dgamma'])
    _within('layernorm_bwd dbeta', what, db[:D], ref['dbeta'], ref['b_dbeta'])
    assert torch.equal(dxb[:M].cpu(), dxf[:M].cpu().to(torch.bfloat16)), 'dxb is not RNE(dxf)'
    want_cs, b_cs = R.colsum(dxb[:M].cpu().float(), presets[2], n_cu)       # of the values the kernel stored
    _within('layernorm_bwd dxb_colsum', what, cs[:D], want_cs, b_cs)
    if planted:                                  # the sums consist of the later trips' rows alone
        rpw = R.ln_bwd_grid(M, n_cu)[1]
        assert float(dy[:rpw].float().abs().max()) == 0.0 and float((ref['dbeta'] - presets[1].double()).abs().max()) > 0.5
    return xbuf, dyb, drb, gamma, presets, dxf, dxb


@pytest.mark.parametrize('with_res', [True, False])
@pytest.mark.parametrize('dy_f32', [False, True])
@pytest.mark.parametrize('mi', range(7))
def test_layernorm_backward(lib, n_cu, mi, dy_f32, with_res):
    M = R.ln_bwd_cases(n_cu)[mi]
    xbuf, dyb, drb, gamma, presets, dxf, dxb = _check_ln_bwd(lib, n_cu, M, dy_f32, with_res, False)
    ldx = xbuf.shape[1]
    if dy_f32 == with_res:                       # half of the cases: the choice of outputs does not move a bit of dx
        f_only = _ln_bwd(lib, xbuf, ldx, dyb, gamma.cuda(), 1e-6, drb, M, presets, want_b=False, colsum=False)
        b_only = _ln_bwd(lib, xbuf, ldx, dyb, gamma.cuda(), 1e-6, drb, M, presets, want_f=False)
        no_cs = _ln_bwd(lib, xbuf, ldx, dyb, gamma.cuda(), 1e-6, drb, M, presets, colsum=False)
        assert _same_bits(f_only[0], dxf) and _same_bits(b_only[1], dxb) and _same_bits(no_cs[0], dxf) and _same_bits(no_cs[1], dxb)


@pytest.mark.parametrize('dy_f32', [False, True])
@pytest.mark.parametrize('mi', [5, 6])
def test_layernorm_backward_later_trips_alone(lib, n_cu, mi, dy_f32):
    """dy is zero in the rows of every wave's first trip: dgamma, dbeta and the column sums consist of the second and third trips."""
    _check_ln_bwd(lib, n_cu, R.ln_bwd_cases(n_cu)[mi], dy_f32, True, True)


# ---------------------------------------------------------------------------------------------------------------------
# cast with column sums
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mi,planted', [(i, False) for i in range(7)] + [(5, True), (6, True)])
def test_cast_bf16_colsum(lib, ops, n_cu, mi, planted):
    """planted (the two sizes at which a wave takes a second trip): x is zero in the rows of every wave's first trip."""
    M = R.ln_bwd_cases(n_cu)[mi]
    rpw = R.ln_bwd_grid(M, n_cu)[1]
    assert not planted or M > rpw
    x = (R._uni((M, D), 6000 + M, 1.5) * (10.0 ** torch.randint(-3, 3, (M, 1), generator=torch.Generator().manual_seed(M)))).float()
    if planted:
        x[:rpw] = 0.0
    preset = R._uni((D,), 61, 2.0).float()
    xbuf, y, cs = _nan_padded(x, M + 1, D), _sent_bf16(M + 1, D), _acc(preset)
    rc = lib.vitcap_cast_bf16_colsum(_p(xbuf), _p(y), _p(cs), M, D, _s())
    assert rc == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    assert _all_sent(y[M:]) and _all_sent(cs[D:])
    assert torch.equal(y[:M].cpu(), x.to(torch.bfloat16)), 'y is not RNE(x)'
    want, b = R.colsum(R.rne_bf16(x), preset, n_cu)
    _within('cast_bf16_colsum colsum', 'M%d%s' % (M, '-planted' if planted else ''), cs[:D], want, b)
    if not planted and M == 1157:
        cs2 = preset.cuda().clone()
        assert _same_bits(ops.cast_bf16_colsum(xbuf[:M], cs2), y[:M])


# ---------------------------------------------------------------------------------------------------------------------
# label-smoothed KL
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kl_ref(case):
    x, tgt, w, preset = R.kl_inputs(case)
    return x, tgt, w, preset, R.ls_kl(x, tgt, case[4], w, preset)


@pytest.mark.parametrize('case', R.KL_CASES, ids=R.kl_case_id)
def test_ls_kl_loss(lib, case):
    V, ldl, ldd, rows, eps, kind, wk, with_grad = case
    x, tgt, w, preset, ref = _kl_ref(case)
    xbuf = _nan_padded(x, rows + 1, ldl)
    dl = _sent_bf16(rows + 1, ldd) if with_grad else None
    loss = _sent_f32(2)
    loss[0] = preset
    tgt_d, w_d = tgt.cuda(), (w.cuda() if w is not None else None)
    rc = lib.vitcap_ls_kl_loss(_p(xbuf), ldl, V, _p(tgt_d), eps, rows, _p(w_d), _p(loss), _p(dl), ldd, _s())
    assert rc == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    assert _all_sent(loss[1:])
    what = R.kl_case_id(case)
    _within('ls_kl loss', what, loss[0], ref['loss'], ref['b_loss'])
    if with_grad:
        assert _all_sent(dl[rows:]), 'the guard row of dlogits was written'
        _within('ls_kl dlogits', what, dl[:rows, :V].float(), ref['grad'], ref['b_grad'])
        assert float(dl[:rows, V:].float().abs().sum()) == 0.0, 'columns V..ldd must be zero'
        if w is not None and float(w[0]) == 0.0:
            assert float(dl[0].float().abs().max()) == 0.0, 'a zero weight gives a zero gradient row'


# ---------------------------------------------------------------------------------------------------------------------
# focal, BCE
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loss_in(B, V, planted):
    return R.loss_inputs(B, V, planted)


def _loss_call(lib, which, x, y, ldl, alpha, preset):
    B, V = x.shape
    xbuf, yb = _nan_padded(x, B + 1, ldl), torch.cat([y.flatten(), torch.full((64,), float('nan'))]).cuda()
    out = _sent_f32(2)
    out[0] = preset
    if which == 'focal':
        rc = lib.vitcap_focal_loss_sum(_p(xbuf), ldl, V, _p(yb), alpha, _p(out), B, _s())
    else:
        rc = lib.vitcap_bce_logits_mean(_p(xbuf), ldl, V, _p(yb), _p(out), B, _s())
    assert rc == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    assert _all_sent(out[1:])
    return out[0]


@pytest.mark.parametrize('B,V,ldl,planted', [c + (False,) for c in R.LOSS_CASES] + [c + (True,) for c in R.LOSS_CASES if c[0] * c[1] > R.LOSS_GRID])
def test_focal_and_bce(lib, B, V, ldl, planted):
    """planted (the sizes at which a thread takes a second trip): the loss sits in flat indices >= 262144 alone."""
    x, y = _loss_in(B, V, planted)
    what = 'B%d-V%d%s' % (B, V, '-planted' if planted else '')
    for alpha in (0.5, 0.25):
        ref = R.focal(x, y, alpha, 1.5)
        _within('focal loss', what + '-a%g' % alpha, _loss_call(lib, 'focal', x, y, ldl, alpha, 1.5), ref['loss'], ref['b_loss'])
    ref = R.bce(x, y, -0.5)
    _within('bce loss', what, _loss_call(lib, 'bce', x, y, ldl, 0.0, -0.5), ref['loss'], ref['b_loss'])
    if planted:
        assert float(x.flatten()[:R.LOSS_GRID].max()) == -40.0 and float(y.flatten()[:R.LOSS_GRID].max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# gradient norm
# ---------------------------------------------------------------------------------------------------------------------
def _sumsq(lib, gbuf, n):
    out = _sent_f32(2)
    rc = lib.vitcap_sumsq(_p(gbuf), n, _p(out), _s())
    assert rc == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    assert _all_sent(out[1:]) and not _all_sent(out[:1]), 'out[0] is overwritten, out[1] is not touched'
    return out[:1].clone()


@pytest.mark.parametrize('n,kind', [(n, k) for n in R.SUMSQ_N for k in R.SUMSQ_KINDS if k != 'second_trip_only' or n > R.SUMSQ_GRID])
def test_sumsq(lib, n, kind):
    g = R.sumsq_input(n, kind)
    ref = R.sumsq(g)
    gbuf = torch.cat([g, torch.full((4,), float('nan'))]).cuda()
    a = _sumsq(lib, gbuf, n)
    _within('sumsq', 'n%d-%s' % (n, kind), a[0], ref['sumsq'], ref['b_sumsq'])
    other = torch.ones(4096, device='cuda')
    _sumsq(lib, other, 4096)                     # an unrelated launch that reuses the partials' scratch
    (other * 2).sum()
    assert _same_bits(_sumsq(lib, gbuf, n), a), 'two calls on the same data must give the same bits'


# ---------------------------------------------------------------------------------------------------------------------
# fused clip + AdamW
# ---------------------------------------------------------------------------------------------------------------------
NCH = len(R.ADAMW_LR_WD)


def _adamw(lib, p, g, m, v, lr_d, wd_d, ss, clip, lr_scale, step):
    rc = lib.vitcap_adamw_multi(_p(p), _p(g), _p(m), _p(v), _p(lr_d), _p(wd_d), _p(ss), clip, lr_scale, step, 0.9, 0.999, 1e-8, NCH, _s())
    assert rc == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()


def _adamw_state(p0):
    """p, m, v of NCH chunks plus a guard chunk of sentinels (behind nchunks: never touched)."""
    st = []
    for init in (p0, torch.zeros_like(p0), torch.zeros_like(p0)):
        t = _sent_f32((NCH + 1) * R.CHUNK)
        t[:NCH * R.CHUNK] = init.cuda()
        st.append(t)
    return st


@pytest.mark.parametrize('name,clip,lr_scale,zero_norm', [
    ('clipped', 1.0, 1.0, False), ('unclipped', 1e4, 1.0, False), ('gsumsq0', 1.0, 1.0, True),
    ('clipped-scale0.37', 1.0, 0.37, False), ('clipped-scale0', 1.0, 0.0, False)])
def test_adamw(lib, name, clip, lr_scale, zero_norm):
    """Steps 1, 2, 3, 1000, 20000 on six chunks; the fp64 reference restarts from the device's own p, m, v before each step."""
    p0, g = R.adamw_inputs()
    n = NCH * R.CHUNK
    G = torch.cat([g, torch.full((R.CHUNK,), float('nan'))]).cuda()
    lr_d = torch.tensor([c[0] for c in R.ADAMW_LR_WD] + [1.0], dtype=torch.float32).cuda()
    wd_d = torch.tensor([c[1] for c in R.ADAMW_LR_WD] + [1.0], dtype=torch.float32).cuda()
    ss = torch.zeros(1, device='cuda')
    if not zero_norm:
        assert lib.vitcap_sumsq(_p(G), n, _p(ss), _s()) == 0
    gsumsq = float(ss.cpu()[0])
    assert zero_norm or (math.sqrt(gsumsq) > clip) == name.startswith('clipped'), gsumsq
    p, m, v = _adamw_state(p0)
    free = _adamw_state(p0) if name in ('unclipped', 'gsumsq0') else None       # the same steps with clip = 1e30
    for step in R.ADAMW_STEPS:
        before = [t[:n].cpu() for t in (p, m, v)]
        _adamw(lib, p, G, m, v, lr_d, wd_d, ss, clip, lr_scale, step)
        for t in (p, m, v):
            assert _all_sent(t[n:]), 'the chunk behind nchunks was touched'
        after = [t[:n].cpu() for t in (p, m, v)]
        for c, (lr, wd) in enumerate(R.ADAMW_LR_WD):
            sl = slice(c * R.CHUNK, (c + 1) * R.CHUNK)
            what = '%s-step%d-lr%g-wd%g' % (name, step, lr, wd)
            if lr == 0.0:
                assert all(_same_bits(after[i][sl], before[i][sl]) for i in range(3)), 'the lr = 0 chunk was touched'
                continue
            ref = R.adamw(before[0][sl], g[sl], before[1][sl], before[2][sl], lr, wd, gsumsq, clip, lr_scale, step)
            _within('adamw p_new-p_old', what, after[0][sl].double() - before[0][sl].double(), ref['dp'], ref['b_dp'])
            _within('adamw m', what, after[1][sl], ref['m'], ref['b_m'])
            _within('adamw v', what, after[2][sl], ref['v'], ref['b_v'])
            if lr_scale == 0.0:
                assert _same_bits(after[0][sl], before[0][sl]), 'lr_scale = 0 must leave p as it is'
                assert not _same_bits(after[1][sl], before[1][sl]) and not _same_bits(after[2][sl], before[2][sl])
        if free is not None:
            _adamw(lib, free[0], G, free[1], free[2], lr_d, wd_d, ss, 1e30, lr_scale, step)
            assert all(_same_bits(a, b) for a, b in zip(free, (p, m, v))), 'below the clip the step is the unclipped one'


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_without_a_write(lib):
    """Where an entry point states a requirement: error returned, nothing written, every output still the sentinel."""
    z = lambda *s: torch.zeros(s, device='cuda')
    out = _sent_f32(2)
    assert lib.vitcap_sumsq(_p(z(8)), 6, _p(out), _s()) != 0 and b'sumsq' in lib.vitcap_last_error()
    p, m, v = _sent_f32(2048), _sent_f32(2048), _sent_f32(2048)
    one = torch.ones(2, device='cuda')
    for step, nch in ((0, 2), (1, 0)):
        rc = lib.vitcap_adamw_multi(_p(p), _p(z(2048)), _p(m), _p(v), _p(one), _p(one), _p(one), 1.0, 1.0, step, 0.9, 0.999, 1e-8, nch, _s())
        assert rc != 0 and b'adamw' in lib.vitcap_last_error()
    loss, dl = _sent_f32(2), _sent_bf16(4, 64)
    tgt = torch.zeros(4, dtype=torch.long, device='cuda')
    for V, rows in ((1, 4), (8, 0)):
        rc = lib.vitcap_ls_kl_loss(_p(z(4, 64)), 64, V, _p(tgt), 0.1, rows, None, _p(loss), _p(dl), 64, _s())
        assert rc != 0 and b'ls_kl' in lib.vitcap_last_error()
    dxf, dxb, dg, db, cs = _sent_f32(4, 1024), _sent_bf16(4, 1024), _sent_f32(1024), _sent_f32(1024), _sent_f32(1024)
    x, dy, gam = z(4, 1024), z(4, 1024), z(1024)
    for Dd, want_b in ((1024, True), (512, True), (768, False)):          # D != 768; column sums without the bf16 output
        rc = lib.vitcap_layernorm_bwd(_p(x), 1024, _p(dy), 1, _p(gam), 1e-6, None, _p(dxf), _p(dxb) if want_b else None, _p(dg), _p(db),
                                      _p(cs), 4, Dd, _s())
        assert rc != 0 and b'layernorm_bwd' in lib.vitcap_last_error()
    y, cs2 = _sent_bf16(4, 1024), _sent_f32(1024)
    for Dd in (1024, 512):
        assert lib.vitcap_cast_bf16_colsum(_p(x), _p(y), _p(cs2), 4, Dd, _s()) != 0 and b'cast_bf16_colsum' in lib.vitcap_last_error()
    torch.cuda.synchronize()
    for t in (out, p, m, v, loss, dl, dxf, dxb, dg, db, cs, y, cs2):
        assert _all_sent(t)
