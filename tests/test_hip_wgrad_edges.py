"""Exact parity of the weight-gradient GEMM (vitcap_gemm_tn, vitcap_gemm_tn_sum) and of its feeders (vitcap_colsum_bf16,
vitcap_transpose_colsum, vitcap_cast_transpose, vitcap_cast_bf16, vitcap_reduce_slabs) with oracle/wgrad_ref.py at ring, split, tile
and stride edges (docs/LAB_tests_wgrad.md).

The entry points are called through ctypes so strides and offset bases can be passed.  Operands sit in guarded buffers: bf16 NaN in
the columns behind the used ones, in four rows in front and in the rows behind M, so a read of any of them shows in the result.
Outputs are pre-filled with the sentinel (fp32 0x7B7B7B7B, bf16 0x7B7B) and followed by a guard that must survive.  On the lattice
operands every sum is exact in fp32 in any order, so ONE torch.equal per case compares the whole guarded buffer with its expected
image: every slab against its own rows, every element, written exactly where it belongs.  Only the two full-mantissa comparisons
carry a bound; each prints its largest err / bound.  tests/test_wgrad_cpu.py proves without a GPU which cases see which mutant.
"""
import ctypes as C

import pytest
import torch

from oracle import wgrad_ref as R

pytestmark = pytest.mark.gpu

FRONT, BACK = 4, 68          # NaN rows in front of an operand and behind its M rows (a whole 64-row step and more)
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
        print('MAXIMUM %-20s err/bound %.3f  (%s)' % ((k,) + MAXIMA[k]))


def _p(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(got, want, what, bits=False):
    """The one comparison of a case: torch.equal of the whole guarded buffer with its image (no NaN in an image: the sentinel is
    finite); bits=True compares the bit patterns instead, which tells -0.0 from 0.0 (the casts)."""
    g, w = got.detach().cpu(), want
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if bits:
        g, w = _bits(g), _bits(w)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError('%s: %d of %d elements differ, first at %s: got %r, want %r' % (
            what, bad.shape[0], g.numel(), i, float(got.detach().cpu()[i]), float(want[i])))


def _all_sent(t):
    b = _bits(t)
    return bool((b == (R.SENT16 if b.dtype == torch.int16 else R.SENT32)).all())


def _within(key, what, got, want, bound):
    got = torch.as_tensor(got, dtype=torch.float64).cpu()
    err = (got - want).abs()
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float('inf')), ratio)
    top = float(ratio.max())
    print('MEASURED %s %s: largest err/bound %.3f' % (key, what, top))
    if key not in MAXIMA or top > MAXIMA[key][0]:
        MAXIMA[key] = (top, what)
    bad = ~(err <= bound)
    assert not bad.any(), '%s %s: %d/%d elements beyond their bound, largest err/bound %.3g' % (key, what, int(bad.sum()), bad.numel(), top)


def _operand(t, ld, col0=0):
    """bf16 [M][W] -> (device buffer [FRONT + M + BACK][ld] of NaN holding t at rows FRONT.., columns col0.., the view of t in it)."""
    M, W = t.shape
    assert col0 + W <= ld
    buf = torch.full((FRONT + M + BACK, ld), float('nan'), dtype=torch.bfloat16)
    buf[FRONT:FRONT + M, col0:col0 + W] = t
    dev = buf.cuda()
    return dev, dev[FRONT:FRONT + M, col0:col0 + W]


def _tn(lib, Y, X, splits, ldy=None, coly=0, ldx=None, colx=0):
    """vitcap_gemm_tn on guarded operands into a sentinel slab buffer with a guard slab; returns the buffer [splits + 1][N][K]."""
    M, N = Y.shape
    K = X.shape[1]
    ldy = N + 8 if ldy is None else ldy
    ldx = K + 16 if ldx is None else ldx
    ybuf, yv = _operand(Y, ldy, coly)
    xbuf, xv = _operand(X, ldx, colx)
    slabs = R.sent_f32(splits + 1, N, K).cuda()
    rc = lib.vitcap_gemm_tn(_p(yv), ldy, _p(xv), ldx, _p(slabs), M, N, K, splits, _s())
    assert rc == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    return slabs


# ---------------------------------------------------------------------------------------------------------------------
# A-D: the GEMM on lattice operands
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.CASES_RING, ids=R.case_id)
def test_ring_lengths_and_row_tails(lib, case):
    """splits = 1: 2, 4, 6, 8, 10, 12 and 20 ring stages, M % 32 in {1, 31, 0} within each; M <= 32 takes its second stage from the zero page."""
    Y, X, image = R.lattice_case(*case)
    _same(_tn(lib, Y, X, 1), image, R.case_id(case))


@pytest.mark.parametrize('case', R.CASES_TILES, ids=R.case_id)
def test_tiles_and_xcd_remap(lib, case):
    """1..18 workgroups with and without a remainder mod 8, tiles_n != tiles_k both ways: every (split, tile) written exactly once."""
    Y, X, image = R.lattice_case(*case)
    _same(_tn(lib, Y, X, case[3]), image, R.case_id(case))


@pytest.mark.parametrize('case', R.CASES_SPLITS, ids=R.case_id)
def test_splits_own_rows_and_empty_splits(lib, case):
    """Every slab against ITS rows; a split without a step (splits > steps included) writes zeros."""
    Y, X, image = R.lattice_case(*case)
    got = _tn(lib, Y, X, case[3])
    _same(got, image, R.case_id(case))
    for s, n in enumerate(R.steps_per_split(case[0], case[3])):
        if n == 0:
            assert int(_bits(got[s]).abs().max()) == 0, 'an empty split writes +0.0'


@pytest.mark.parametrize('case', R.CASES_STRIDES, ids=lambda c: R.case_id(c) + '-ldy%d-ldx%d' % (c[4], c[6]))
def test_strides_and_offset_bases(lib, ops, case):
    """Y as one third of a [M][776] buffer, X as columns 512.. of [M][1040]; and ldy = N, ldx = K, the wrappers' call, bit-equal to it."""
    M, N, K, splits, ldy, coly, ldx, colx = case
    Y, X, image = R.lattice_case(M, N, K, splits)
    got = _tn(lib, Y, X, splits, ldy, coly, ldx, colx)
    _same(got, image, R.case_id(case))
    if ldy == N and ldx == K:
        _same(ops.gemm_tn(Y.cuda(), X.cuda(), splits), image[:splits], R.case_id(case) + ' ops.gemm_tn')


# ---------------------------------------------------------------------------------------------------------------------
# E: full-mantissa operands
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.CASES_FULL, ids=R.case_id)
def test_full_mantissa_operands(lib, case):
    M, N, K, splits = case
    Y, X = R.full_mantissa(*case)
    ref, mag, rows = R.slab_abs_ref(Y, X, splits)
    got = _tn(lib, Y, X, splits)
    assert _all_sent(got[splits]), 'the guard slab was written'
    _within('gemm_tn', R.case_id(case), got[:splits], ref, R.gemm_bound(mag, rows))


# ---------------------------------------------------------------------------------------------------------------------
# F: the in-launch sum.  It waits across workgroups: at most 20 of them, the current stream only, nothing else in flight.
# ---------------------------------------------------------------------------------------------------------------------
def _tn_sum(lib, yv, ldy, xv, ldx, slabs, out, accumulate, M, N, K, splits):
    rc = lib.vitcap_gemm_tn_sum(_p(yv), ldy, _p(xv), ldx, _p(slabs), _p(out), int(accumulate), M, N, K, splits, _s())
    assert rc == 0, lib.vitcap_last_error()


@pytest.mark.parametrize('accumulate', [False, True], ids=['plain', 'accumulate'])
@pytest.mark.parametrize('case', R.CASES_SUM, ids=R.case_id)
def test_sum_in_launch(lib, case, accumulate):
    M, N, K, splits = case
    assert R.workgroups(N, K, splits) <= R.SUM_MAX_WORKGROUPS
    Y, X, image = R.lattice_case(*case)
    preset = R.lattice_preset(N, K, M + splits)
    exact = image[:splits].double().sum(0) + (preset.double() if accumulate else 0)
    want = R.sent_f32(N + 1, K)                                   # out with a guard row
    want[:N] = exact.float()
    assert torch.equal(want[:N].double(), exact)                   # the sum and the preset stay on the lattice
    ybuf, yv = _operand(Y, N + 8)
    xbuf, xv = _operand(X, K + 16)
    outs = []
    for fused in (True, False):
        out = R.sent_f32(N + 1, K)
        if accumulate:
            out[:N] = preset
        out = out.cuda()
        slabs = R.sent_f32(splits + 1, N, K).cuda()
        torch.cuda.synchronize()
        if fused:
            _tn_sum(lib, yv, N + 8, xv, K + 16, slabs, out, accumulate, M, N, K, splits)
        else:
            assert lib.vitcap_gemm_tn(_p(yv), N + 8, _p(xv), K + 16, _p(slabs), M, N, K, splits, _s()) == 0, lib.vitcap_last_error()
            assert lib.vitcap_reduce_slabs(_p(slabs), N * K, splits, _p(out), N * K, int(accumulate), _s()) == 0, lib.vitcap_last_error()
        torch.cuda.synchronize()
        assert _all_sent(slabs[splits]), 'the guard slab was written'
        outs.append(out)
    _same(outs[0], want, R.case_id(case) + ' gemm_tn_sum against the exact sum')
    _same(outs[1], want, R.case_id(case) + ' gemm_tn + reduce_slabs against the exact sum')


def test_sum_ticket_slots_are_reused(lib):
    """130 launches go twice round the launcher's 64 ticket slots: each must find its tickets at zero and leave them so.  Every launch is
    compared on the device; one host synchronisation at the end.  Slot reuse, not a stress loop: the count stays."""
    M, N, K, splits = R.SUM_REUSE
    Y, X, image = R.lattice_case(*R.SUM_REUSE)
    want = image[:splits].sum(0).cuda()
    ybuf, yv = _operand(Y, N + 8)
    xbuf, xv = _operand(X, K + 16)
    slabs = R.sent_f32(splits + 1, N, K).cuda()
    out = R.sent_f32(N + 1, K).cuda()
    wrong = torch.zeros((), dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    for _ in range(R.SUM_REUSE_LAUNCHES):
        out.view(torch.int32).fill_(R.SENT32)
        _tn_sum(lib, yv, N + 8, xv, K + 16, slabs, out, False, M, N, K, splits)
        wrong += (out[:N] != want).any()
    torch.cuda.synchronize()
    assert int(wrong) == 0, '%d of %d launches gave another sum' % (int(wrong), R.SUM_REUSE_LAUNCHES)
    assert _all_sent(out[N:]) and _all_sent(slabs[splits])


# ---------------------------------------------------------------------------------------------------------------------
# G: refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_gemm_refusals(lib, n_cu):
    M = 64
    ybuf, yv = _operand(torch.ones(M, 512, dtype=torch.bfloat16), 520)
    xbuf, xv = _operand(torch.ones(M, 512, dtype=torch.bfloat16), 528)
    slabs = R.sent_f32(n_cu + 2, 256, 256).cuda()       # room for what the last refusal would write if it were not refused
    out = R.sent_f32(256, 256).cuda()
    tn, tsum = lib.vitcap_gemm_tn, lib.vitcap_gemm_tn_sum
    refused = {
        'N = 128': lambda: tn(_p(yv), 520, _p(xv), 528, _p(slabs), M, 128, 256, 1, _s()),
        'K = 384': lambda: tn(_p(yv), 520, _p(xv), 528, _p(slabs), M, 256, 384, 1, _s()),
        'ldy = N + 4': lambda: tn(_p(yv), 260, _p(xv), 528, _p(slabs), M, 256, 256, 1, _s()),
        'Y base 8 bytes off': lambda: tn(_p(yv, 8), 520, _p(xv), 528, _p(slabs), M, 256, 256, 1, _s()),
        'splits = 0': lambda: tn(_p(yv), 520, _p(xv), 528, _p(slabs), M, 256, 256, 0, _s()),
        'M = 0': lambda: tn(_p(yv), 520, _p(xv), 528, _p(slabs), 0, 256, 256, 1, _s()),
        'sum, out = NULL': lambda: tsum(_p(yv), 520, _p(xv), 528, _p(slabs), None, 0, M, 256, 256, 1, _s()),
        'sum, more workgroups than CUs': lambda: tsum(_p(yv), 520, _p(xv), 528, _p(slabs), _p(out), 0, M, 256, 256, n_cu + 1, _s()),
    }
    for what, call in refused.items():
        assert call() != 0 and lib.vitcap_last_error(), what + ' was accepted'
        torch.cuda.synchronize()
        assert bool((slabs.view(torch.int32) == R.SENT32).all()) and _all_sent(out), what + ': refused, yet an output was written'
    assert tsum(_p(yv), 520, _p(xv), 528, _p(slabs), _p(out), 0, M, 256, 256, 1, _s()) == 0      # the same arguments, one workgroup: accepted
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# H: the feeders
# ---------------------------------------------------------------------------------------------------------------------
def _preset_guarded(n, preset, guard=16):
    t = R.sent_f32(n + guard)
    t[:n] = preset
    return t


@pytest.mark.parametrize('M', R.COLSUM_M)
@pytest.mark.parametrize('N', R.COLSUM_N)
def test_colsum(lib, N, M):
    y = R.colsum_lattice(M, N)
    ybuf, yv = _operand(y, N + 8)
    out = _preset_guarded(N, R.COLSUM_PRESET).cuda()
    assert lib.vitcap_colsum_bf16(_p(yv), N + 8, M, N, _p(out), _s()) == 0, lib.vitcap_last_error()
    want = _preset_guarded(N, R.colsum_ref(y, R.COLSUM_PRESET).float())
    _same(out, want, 'colsum M%d N%d' % (M, N))


def test_colsum_full_mantissa_and_refusals(lib):
    M, N = R.COLSUM_FULL
    y = R.colsum_full(M, N)
    ybuf, yv = _operand(y, N + 8)
    out = _preset_guarded(N, R.COLSUM_PRESET).cuda()
    assert lib.vitcap_colsum_bf16(_p(yv), N + 8, M, N, _p(out), _s()) == 0, lib.vitcap_last_error()
    assert _all_sent(out[N:])
    _within('colsum', 'M%d-N%d' % (M, N), out[:N], R.colsum_ref(y, R.COLSUM_PRESET), R.colsum_bound(y, R.COLSUM_PRESET))
    out = _preset_guarded(16, R.COLSUM_PRESET).cuda()
    before = out.clone()
    assert lib.vitcap_colsum_bf16(_p(yv), N + 8, M, 12, _p(out), _s()) != 0, 'N = 12 was accepted'
    assert lib.vitcap_colsum_bf16(_p(yv), 12, M, 8, _p(out), _s()) != 0, 'ldy = N + 4 was accepted'
    _same(out, before.cpu(), 'colsum refusals')


@pytest.mark.parametrize('with_colsum', [True, False], ids=['colsum', 'nocolsum'])
@pytest.mark.parametrize('extra', [0, 64], ids=['ldt', 'ldt+64'])
@pytest.mark.parametrize('Cc', R.TRANSPOSE_C)
@pytest.mark.parametrize('Rr', R.TRANSPOSE_R)
def test_transpose_colsum(lib, Rr, Cc, extra, with_colsum):
    x = R.transpose_input(Rr, Cc)
    ldt = R.ceil_to(Rr, 64) + extra
    xbuf, xv = _operand(x, Cc + 8)
    xt = R.sent_bf16(Cc + 2, ldt).cuda()
    cs = _preset_guarded(Cc, 0.5).cuda()
    rc = lib.vitcap_transpose_colsum(_p(xv), Cc + 8, _p(xt), ldt, _p(cs) if with_colsum else None, Rr, Cc, _s())
    assert rc == 0, lib.vitcap_last_error()
    what = 'transpose R%d C%d ldt%d' % (Rr, Cc, ldt)
    _same(xt, R.transpose_image(x, ldt), what, bits=True)
    _same(cs, _preset_guarded(Cc, R.colsum_ref(x, 0.5).float() if with_colsum else 0.5), what + ' column sums')


def test_transpose_refusals(lib):
    x = R.transpose_input(130, 192)
    xbuf, xv = _operand(x, 200)
    xt = R.sent_bf16(194, 192).cuda()
    cs = _preset_guarded(192, 0.5).cuda()
    before = cs.clone().cpu()
    for what, (Rr, Cc, ldt) in {'C = 96': (64, 96, 64), 'ldt = 96': (64, 64, 96), 'ldt < R': (130, 64, 128)}.items():
        assert lib.vitcap_transpose_colsum(_p(xv), 200, _p(xt), ldt, _p(cs), Rr, Cc, _s()) != 0, what + ' was accepted'
    assert _all_sent(xt)
    _same(cs, before, 'transpose refusals')


@pytest.mark.parametrize('mode', ['w', 'wt', 'both'])
@pytest.mark.parametrize('extra', [0, 8], ids=['ldt', 'ldt+8'])
@pytest.mark.parametrize('K', R.CT_K)
@pytest.mark.parametrize('N', R.CT_N)
def test_cast_transpose(lib, N, K, extra, mode):
    w = R.cast_values(N * K, N * 131 + K).view(N, K)
    ldt = R.ceil_to(N, 8) + extra
    want_w, want_t = R.cast_transpose_images(w, ldt)
    assert torch.equal(_bits(want_w[:N]), _bits(w.to(torch.bfloat16)))                 # torch's own rounding, inf and -0.0 included
    wd = torch.cat([w.reshape(-1), torch.full((64,), float('nan'))]).cuda()
    wb = R.sent_bf16(N + 1, K).cuda() if mode != 'wt' else None
    wt = R.sent_bf16(K + 1, ldt).cuda() if mode != 'w' else None
    assert lib.vitcap_cast_transpose(_p(wd), _p(wb), _p(wt), N, K, ldt, _s()) == 0, lib.vitcap_last_error()
    what = 'cast_transpose N%d K%d ldt%d %s' % (N, K, ldt, mode)
    if wb is not None:
        _same(wb, want_w, what + ' w_bf16', bits=True)
    if wt is not None:
        _same(wt, want_t, what + ' wt_bf16', bits=True)
        assert torch.equal(_bits(wt[:K, :N]), _bits(w.to(torch.bfloat16).t()))


def test_cast_transpose_refusals(lib):
    w = R.cast_values(64 * 96, 5).cuda()
    wb, wt = R.sent_bf16(65, 96).cuda(), R.sent_bf16(97, 72).cuda()
    for what, (N, K, ldt) in {'K = 96': (64, 96, 64), 'ldt < N': (64, 64, 56), 'ldt = N + 4': (64, 64, 68)}.items():
        assert lib.vitcap_cast_transpose(_p(w), _p(wb), _p(wt), N, K, ldt, _s()) != 0, what + ' was accepted'
    assert _all_sent(wb) and _all_sent(wt)


@pytest.mark.parametrize('n', R.CAST_N)
def test_cast_bf16(lib, n):
    v = R.cast_values(n, 7000 + n)
    xd = torch.cat([v, torch.full((16,), float('nan'))]).cuda()
    y = R.sent_bf16(n + 16).cuda()
    assert lib.vitcap_cast_bf16(_p(xd), _p(y), n, _s()) == 0, lib.vitcap_last_error()
    want = R.sent_bf16(n + 16)
    want[:n] = R.rne_bf16(v)
    _same(y, want, 'cast_bf16 n%d' % n, bits=True)
    assert torch.equal(_bits(y[:n]), _bits(v.to(torch.bfloat16)))


@pytest.mark.parametrize('accumulate', [False, True], ids=['plain', 'accumulate'])
@pytest.mark.parametrize('n', R.REDUCE_N)
@pytest.mark.parametrize('S', R.REDUCE_S)
def test_reduce_slabs(lib, S, n, accumulate):
    v, pre = R.reduce_values(S, n, S * 10007 + n)
    stride = n + 256
    buf = torch.full((S, stride), float('nan'))
    buf[:, :n] = v
    out, buf = _preset_guarded(n, pre).cuda(), buf.cuda()
    assert lib.vitcap_reduce_slabs(_p(buf), stride, S, _p(out), n, int(accumulate), _s()) == 0, lib.vitcap_last_error()
    _same(out, _preset_guarded(n, R.reduce_slabs_f32(v, pre, accumulate)), 'reduce_slabs S%d n%d' % (S, n), bits=True)


def test_reduce_slabs_refusals(lib):
    buf = torch.zeros(2, 264).cuda()
    out = R.sent_f32(24).cuda()
    assert lib.vitcap_reduce_slabs(_p(buf), 264, 2, _p(out), 6, 0, _s()) != 0, 'n = 6 was accepted'
    assert lib.vitcap_reduce_slabs(_p(buf), 264, 0, _p(out), 8, 0, _s()) != 0, 'S = 0 was accepted'
    assert _all_sent(out)
