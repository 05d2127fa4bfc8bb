"""Every launch form of vitcap_gemm_bias_act / vitcap_gemm_ex against an independent CPU reference, at tile, stride and k-ring edges
(docs/LAB_tests_gemm_forms.md).

Operands sit on an exact lattice: A holds integers in -3..3, W integers in -3..3 times 2^-5, bias / residual multiples of 2^-5 in +-4.
Every product and partial sum is then a multiple of 2^-10 below 2^10: 20 bits of significand, so fp32 accumulation is exact in any order
and an un-activated output must EQUAL the fp64 reference (fp32 output) or its round-to-nearest-even bf16 cast, bit for bit.  Random
lattice operands reveal position: a misplaced row, column, k-tile, bias quad or residual row changes some element.

Guards: every buffer sits inside a larger allocation.  Around A and W (a row in front, the rows behind, the columns behind K) lies
bf16 NaN, so a fragment read from padding poisons the output; outputs are pre-filled with a sentinel bit pattern (bf16 0x7B7B, fp32
0x7B7B7B7B) that must survive in the ldc gap, in front of row 0, behind row M, in the rows a row map skips and behind the last slab.
Every exact comparison is ONE torch.equal of the whole guarded buffer with its expected image.

Toleranced comparisons (activations, aux / zout, column sums, row statistics' exp sums, full-mantissa operands) print their largest
error / bound ratio (`pytest -s`): the lab note's figures.
"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SENT16 = 0x7B7B
SENT32 = 0x7B7B7B7B
ACT_NONE, ACT_GELU, ACT_TANH = 0, 1, 2

# tile_hint -> (tile rows, tile columns, family).  The hint ledger (test_hint_ledger) holds vitcap_gemm_ex to exactly these keys.
FORMS = {
    0: (None, None, 'auto'),
    1: (64, 64, 'ring'), 2: (128, 128, 'lds2'), 13: (64, 32, 'ring'), 14: (32, 32, 'ring'), 15: (32, 64, 'ring'),
    4: (None, 32, 'skinny'),
    20: (64, 32, 'resident'), 21: (32, 32, 'resident'), 22: (32, 64, 'resident'),
    23: (64, 32, 'ringslab'), 24: (32, 32, 'ringslab'),
    5: (256, 256, '8wave'), 30: (192, 256, '8wave'), 31: (128, 256, '8wave'), 32: (256, 256, '8wave'), 33: (256, 256, '8wave'),
    40: (256, 256, '4wave'), 41: (256, 256, '4wave'), 42: (256, 256, '4wave'),
}


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vitcap_amd import ops as o
    return o


@pytest.fixture(scope='module')
def lib(ops):
    from vitcap_amd._lib import lib as l
    return l


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


MEASURED = {}


def _measure(what, err, bound):
    """Largest error / bound ratio of a toleranced comparison, printed and kept per `what`; asserts err <= bound everywhere."""
    err, bound = err.double().flatten(), bound.double().flatten()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    i = int(err.argmax()) if err.numel() else 0
    MEASURED[what] = max(MEASURED.get(what, 0.0), ratio)
    print('MEASURED %s: max err %.3e (bound there %.3e), largest err/bound %.3g' % (what, float(err[i]), float(bound[i]), ratio))
    bad = ~(err <= bound)                     # a NaN (or a left-over sentinel) is bad
    assert not bad.any(), '%s: %d/%d elements off, largest err/bound %.3g' % (what, int(bad.sum()), bad.numel(), ratio)


# ------------------------------------------------------------------------------------------------ operands
def _lat(shape, g, lo=-128, hi=128):
    """multiples of 2^-5 in +-4 (bias, residual, aux)"""
    return torch.randint(lo, hi + 1, shape, generator=g).double() / 32


class Problem(object):
    """A [M,K], W [N,K], bias [N] on the CPU in fp64 (every value exactly representable in its device type) and A @ W^T."""

    def __init__(self, M, N, K, seed=0, full=False):
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * N + K)
        self.M, self.N, self.K, self.full, self.g = M, N, K, full, g
        if full:      # full-mantissa operands: bits the lattice does not exercise
            self.A = torch.randn((M, K), generator=g).to(torch.bfloat16).double()
            self.W = (0.05 * torch.randn((N, K), generator=g)).to(torch.bfloat16).double()
            self.bias = torch.randn((N,), generator=g).float().double()
        else:
            self.A = torch.randint(-3, 4, (M, K), generator=g).double()
            self.W = torch.randint(-3, 4, (N, K), generator=g).double() / 32
            self.bias = _lat((N,), g)
        self._acc = None
        self._dev = {}

    @property
    def acc(self):
        if self._acc is None:
            self._acc = self.A @ self.W.T
        return self._acc

    def extra(self, rows):
        """residual / aux values for `rows` rows"""
        if self.full:
            return torch.randn((rows, self.N), generator=self.g).float().double()
        return _lat((rows, self.N), self.g)

    def dev_operand(self, which, ld):
        """A or W on the device inside a NaN frame: one guard row in front, two behind, columns K..ld-1; returns (buffer, pointer)"""
        key = (which, ld)
        if key not in self._dev:
            v = self.A if which == 'A' else self.W
            buf = torch.full((v.shape[0] + 3, ld), float('nan'), dtype=torch.bfloat16)
            buf[1:1 + v.shape[0], :self.K] = v.to(torch.bfloat16)
            self._dev[key] = buf.cuda()
        d = self._dev[key]
        return d, d.data_ptr() + ld * 2


def _dev_vec(v):
    """fp32 vector on the device, 4 NaN floats in front and behind; returns (buffer, pointer)"""
    buf = torch.full((v.numel() + 8,), float('nan'), dtype=torch.float32)
    buf[4:4 + v.numel()] = v.float()
    d = buf.cuda()
    return d, d.data_ptr() + 16


def _sent(rows, ld, f32, device='cuda'):
    if f32:
        return torch.full((rows, ld), SENT32, dtype=torch.int32, device=device).view(torch.float32)
    return torch.full((rows, ld), SENT16, dtype=torch.int16, device=device).view(torch.bfloat16)


def _gelu(x):
    return x * 0.5 * torch.special.erfc(-x / math.sqrt(2.0))


def _gelu_grad(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _rows(M, rowmap):
    """(output row of every GEMM row, residual row of every GEMM row, rows of the output buffer)"""
    r = torch.arange(M)
    if not rowmap:
        return r, r, M
    rg, ogr, off, periodic = rowmap
    orow = (r // rg) * ogr + off + r % rg
    rrow = (r % rg) if periodic else orow
    return orow, rrow, ((M + rg - 1) // rg) * ogr + off + 1


G = 4     # guard rows in front of an output (4 rows of a bf16 output with ldc % 8 == 4 keep its base 16-byte aligned)


class Result(object):
    pass


def _run(lib, P, hint=0, f32=True, act=ACT_NONE, bias=True, res=None, pads=(0, 0, 0, 0), rowmap=None, split_k=0, kranges=None,
         live=None, aux=False, zout=False, colsum=False):
    """One launch.  res: None / 'sep' (a buffer of its own) / 'inplace' (C holds the residual).  pads = (lda - K, ldw - K, ldc - N,
    ldr - N).  kranges: the k range of every raw fp32 slab the launch writes (C = [slabs][M][ldc]); the reference is then the
    product over each range.  Returns the device's guarded buffers (on the CPU) next to the fp64 reference."""
    from vitcap_amd._lib import GemmDesc
    M, N, K = P.M, P.N, P.K
    lda, ldw, ldc, ldr = K + pads[0], K + pads[1], N + pads[2], N + pads[3]
    orow, rrow, out_rows = _rows(M, rowmap)
    S = len(kranges) if kranges else 1
    R = S * out_rows
    keep = []
    abuf, aptr = P.dev_operand('A', lda)
    wbuf, wptr = P.dev_operand('W', ldw)
    bptr = None
    if bias:
        bbuf, bptr = _dev_vec(P.bias)
        keep.append(bbuf)
    cbuf = _sent(G + R + 2, ldc, f32)
    cptr = cbuf.data_ptr() + G * ldc * cbuf.element_size()
    resv, rptr = None, None
    if res == 'inplace':
        assert f32 and not rowmap and S == 1
        resv = P.extra(M)
        cbuf[G:G + M, :N] = resv.float().cuda()
        rptr, ldr = cptr, ldc
    elif res == 'sep':
        res_rows = rowmap[0] if (rowmap and rowmap[3]) else out_rows
        resv = P.extra(res_rows)
        rb = torch.full((res_rows + 2, ldr), float('nan'), dtype=torch.float32)
        rb[1:1 + res_rows, :N] = resv.float()
        rb = rb.cuda()
        keep.append(rb)
        rptr = rb.data_ptr() + ldr * 4
    auxv, auxptr, ldaux = None, None, 0
    if aux:
        ldaux = N + 8
        auxv = _lat((M, N), P.g)
        ab = torch.full((M + 2, ldaux), float('nan'), dtype=torch.bfloat16)
        ab[1:1 + M, :N] = auxv.to(torch.bfloat16)
        ab = ab.cuda()
        keep.append(ab)
        auxptr = ab.data_ptr() + ldaux * 2
    zbuf, zptr, ldz = None, None, 0
    if zout:
        ldz = N + 16
        zbuf = _sent(M + 2, ldz, False)
        zptr = zbuf.data_ptr() + ldz * 2
    csbuf, cs0 = None, None
    if colsum:
        cs0 = _lat((N,), P.g)
        csbuf = _sent(1, N + 8, True).flatten()
        csbuf[4:4 + N] = cs0.float().cuda()
    livebuf = None
    if live is not None:
        livebuf = torch.tensor([live, 0, 0, 0], dtype=torch.int32, device='cuda')
    d = GemmDesc(M=M, N=N, K=K, lda=lda, ldw=ldw, ldc=ldc, ldr=ldr if res else 0, act=act, out_dtype=1 if f32 else 0,
                 row_group=rowmap[0] if rowmap else 0, out_group_rows=rowmap[1] if rowmap else 0, out_row_off=rowmap[2] if rowmap else 0,
                 res_periodic=rowmap[3] if rowmap else 0, tile_hint=hint, split_k=split_k,
                 live=livebuf.data_ptr() if livebuf is not None else None, colsum=csbuf.data_ptr() + 16 if colsum else None)
    r = Result()
    # what vitcap_gemm_plan says this very launch is (host query): family, template arguments, grid
    from vitcap_amd._lib import GemmPlanInfo
    r.plan = GemmPlanInfo()
    r.plan_rc = lib.vitcap_gemm_plan(C.byref(d), int(bptr is not None), int(rptr is not None), int(auxptr is not None), ldaux, int(zptr is not None), ldz,
                                     C.byref(r.plan))
    r.plan_err = lib.vitcap_last_error() if r.plan_rc != 0 else b''
    r.family = GemmPlanInfo.FAMILIES[r.plan.family] if r.plan_rc == 0 else None
    r.rc = lib.vitcap_gemm_ex(C.c_void_p(aptr), C.c_void_p(wptr), C.c_void_p(bptr) if bptr else None, C.c_void_p(rptr) if rptr else None,
                              C.c_void_p(cptr), C.byref(d), C.c_void_p(auxptr) if auxptr else None, ldaux,
                              C.c_void_p(zptr) if zptr else None, ldz, _s())
    r.err = lib.vitcap_last_error() if r.rc != 0 else b''
    assert (r.plan_rc, r.plan_err) == (r.rc, r.err), 'vitcap_gemm_plan and vitcap_gemm_ex disagree: %d %r / %d %r' % (r.plan_rc, r.plan_err, r.rc, r.err)
    torch.cuda.synchronize()
    r.f32, r.M, r.N, r.ldc, r.S, r.out_rows, r.orow = f32, M, N, ldc, S, out_rows, orow
    r.C = cbuf.cpu()
    r.Z = zbuf.cpu() if zout else None
    r.colsum = csbuf.cpu() if colsum else None
    r.cs0 = cs0
    # ---- fp64 reference
    if kranges:
        r.ref = torch.stack([P.A[:, k0:k1] @ P.W[:, k0:k1].T for (k0, k1) in kranges])
        r.mag = torch.stack([P.A[:, k0:k1].abs() @ P.W[:, k0:k1].abs().T for (k0, k1) in kranges]) if P.full else None
    else:
        pre = P.acc + (P.bias if bias else 0.0)
        mag = (P.A.abs() @ P.W.abs().T + (P.bias.abs() if bias else 0.0)) if P.full else None
        if aux:
            pre = pre * auxv
        r.pre = pre
        ref = _gelu(pre) if act == ACT_GELU else (torch.tanh(pre) if act == ACT_TANH else pre)
        if res:
            ref = ref + resv[rrow]
            if P.full:
                mag = mag + resv[rrow].abs()
        r.ref, r.mag = ref[None], (mag[None] if P.full else None)
    r.mask = torch.zeros((G + R + 2, ldc), dtype=torch.bool)
    r.ref_img = torch.zeros((G + R + 2, ldc), dtype=torch.float64)
    r.mag_img = torch.zeros((G + R + 2, ldc), dtype=torch.float64) if P.full else None
    for s in range(S):
        rows = G + s * out_rows + orow
        r.mask[rows, :N] = True
        r.ref_img[rows, :N] = r.ref[s]
        if P.full:
            r.mag_img[rows, :N] = r.mag[s]
    del keep
    return r


def _sentinels_outside(r, what):
    bits = r.C.view(torch.int32 if r.f32 else torch.int16)
    assert bool((bits[~r.mask] == (SENT32 if r.f32 else SENT16)).all()), '%s: a sentinel outside the documented output region was overwritten' % what


def _exact(r, what):
    """the whole guarded output buffer against its expected image: sentinel outside the output region, the exact reference inside"""
    assert r.rc == 0, '%s refused: %s' % (what, r.err)
    exp = _sent(r.C.shape[0], r.ldc, r.f32, device='cpu')
    exp[r.mask] = r.ref_img[r.mask].float().to(exp.dtype)
    if not torch.equal(r.C, exp):
        bad = (r.C.float() != exp.float()) | (r.C.float() != r.C.float())
        idx = bad.nonzero()
        raise AssertionError('%s: %d elements of the guarded output differ from the exact reference; first (buffer row, column): %s; got %s want %s'
                             % (what, int(bad.sum()), idx[:6].tolist(), r.C[bad][:6].tolist(), exp[bad][:6].tolist()))


def _act_delta(ref):
    """the accuracy common.h states for gelu_erf2 (7e-7 absolute, 5e-6 relative), as the issue rounds it up"""
    return 6e-6 * ref.abs() + 1e-6


def _within(what, got, ref, delta, f32):
    """`got` against the fp64 reference `ref` when the device's fp32 value is accurate to `delta` BEFORE the output rounding.
    fp32 output: |got - ref| <= delta.  bf16 output: the output rounding is modelled exactly instead of being given a relative
    allowance -- round-to-nearest-even is monotonic, so got must lie in [bf16(ref - delta), bf16(ref + delta)]; nearly everywhere that
    interval is one value.  (Half a bf16 ulp is between 2^-9 and 2^-8 of |ref|, so `2^-9 |ref| + delta` is not met by a correctly
    rounded result: a CPU round-to-nearest of the fp64 GELU reaches 1.67 x that figure.  The ratio against it is printed as
    `literal`; the asserted ratio is the distance of ref from the values that round to `got`, over delta.)"""
    ref, delta = ref.double().flatten(), delta.double().flatten()
    g = got.double().flatten()
    if f32:
        return _measure(what, (g - ref).abs(), delta)
    lo = (ref - delta).float().to(torch.bfloat16).double()
    hi = (ref + delta).float().to(torch.bfloat16).double()
    half_ulp = torch.ldexp(torch.ones_like(g), torch.frexp(g)[1] - 9)          # |g| in [2^(e-1), 2^e): 8 significant bits
    excess = ((g - ref).abs() - half_ulp).clamp_min(0.0)
    ratio = float((excess / delta.clamp_min(1e-300)).max()) if g.numel() else 0.0
    literal = float(((g - ref).abs() / (2.0 ** -9 * ref.abs() + delta).clamp_min(1e-300)).max()) if g.numel() else 0.0
    MEASURED[what] = max(MEASURED.get(what, 0.0), ratio)
    MEASURED[what + ' (literal 2^-9 form)'] = max(MEASURED.get(what + ' (literal 2^-9 form)', 0.0), literal)
    print('MEASURED %s: largest (distance to the rounding interval of got) / delta %.3g; literal err / (2^-9 |ref| + delta) %.3g' % (what, ratio, literal))
    bad = ~((g >= lo) & (g <= hi))            # a NaN (or a left-over sentinel) is bad
    assert not bad.any(), '%s: %d/%d elements outside [bf16(ref - delta), bf16(ref + delta)]; first: got %s ref %s delta %s' % (
        what, int(bad.sum()), bad.numel(), g[bad][:4].tolist(), ref[bad][:4].tolist(), delta[bad][:4].tolist())


def _close_act(r, what):
    """activated (or aux-scaled) output: sentinels outside the region; inside, the fp64 function of the exact pre-activation"""
    assert r.rc == 0, '%s refused: %s' % (what, r.err)
    _sentinels_outside(r, what)
    ref = r.ref_img[r.mask]
    _within(what, r.C[r.mask], ref, _act_delta(ref), r.f32)


def _close_full(r, K, what):
    """full-mantissa operands: the fp32 value within (K + 2) 2^-23 (|A| |W|^T + |bias| + |residual|) of the fp64 reference"""
    assert r.rc == 0, '%s refused: %s' % (what, r.err)
    _sentinels_outside(r, what)
    _within(what, r.C[r.mask], r.ref_img[r.mask], (K + 2) * 2.0 ** -23 * r.mag_img[r.mask], r.f32)


def _refused(r, what, needle=b'gemm'):
    assert r.rc != 0, '%s was not refused' % what
    assert r.err and needle in r.err, r.err
    bits = r.C.view(torch.int32 if r.f32 else torch.int16)
    assert bool((bits == (SENT32 if r.f32 else SENT16)).all()), '%s: refused, but C was written' % what


def _edges(x):
    return [1, x - 1, x, x + 1, 2 * x + 1]


ROWMAP = (5, 7, 1)       # M = 23: groups of 5 rows land 7 apart from row 1 on; the last group is partial
STRIDES = (8, 16, 4, 12)  # lda = K + 8, ldw = K + 16, ldc = N + 4, ldr = N + 12


def _variants(lib, P, hint, what, tanh=True, pads=STRIDES):
    """the epilogue variants of one form at one shape, every operand strided"""
    _exact(_run(lib, P, hint, f32=False, pads=pads), what + ' bf16')
    _close_act(_run(lib, P, hint, f32=False, act=ACT_GELU, pads=pads), what + ' bf16+gelu')
    if tanh:
        _close_act(_run(lib, P, hint, f32=False, act=ACT_TANH, pads=pads), what + ' bf16+tanh')
    _exact(_run(lib, P, hint, f32=True, res='sep', pads=pads), what + ' fp32+residual')
    _exact(_run(lib, P, hint, f32=False, res='sep', pads=pads), what + ' bf16+residual')


def _rowmaps(lib, hint, what, maps=((23, ROWMAP),), N=36, K=128):
    for M, rm in maps:
        P = Problem(M, N, K, seed=hint)
        for periodic in (0, 1):
            _exact(_run(lib, P, hint, f32=True, res='sep', rowmap=rm + (periodic,), pads=STRIDES), '%s row map %s periodic=%d' % (what, rm, periodic))
        _exact(_run(lib, P, hint, f32=False, rowmap=rm + (0,), pads=(0, 0, 4, 0)), '%s row map %s bf16' % (what, rm))


# ------------------------------------------------------------------------------------------------ a. ring and LDS-staged forms
# (name, tile_hint, BM, BN, M values, 4-stage ring?)
RING_FORMS = [
    ('h14_32x32', 14, 32, 32, _edges(32), True),
    ('h13_64x32', 13, 64, 32, _edges(64), True),
    ('h15_32x64', 15, 32, 64, _edges(32), True),
    ('h1_64x64', 1, 64, 64, _edges(64), True),
    ('h2_128x128', 2, 128, 128, _edges(128), False),
    ('auto_M<=128_32x32', 0, 32, 32, _edges(32), True),
    ('auto_M<=256_64x64', 0, 64, 64, [129, 191, 192, 193, 256], True),
    ('auto_M>256_64x64', 0, 64, 64, [257, 319, 320, 321, 513], True),     # the cost model's choice at these grids (t64 < t128)
]


@pytest.mark.parametrize('name,hint,BM,BN,Ms,ring4', RING_FORMS, ids=[f[0] for f in RING_FORMS])
def test_ring_forms(lib, name, hint, BM, BN, Ms, ring4):
    Ns = [4, BN - 4, BN, BN + 4, 2 * BN + 4]
    for M in Ms:                                        # the M x N cross: fp32 + bias at K = 128
        for N in Ns:
            _exact(_run(lib, Problem(M, N, 128, seed=hint), hint), '%s %dx%dx128 fp32+bias' % (name, M, N))
    m1 = Ms[3]                                          # BM + 1 (auto forms: the value just past a tile edge inside the form's M range)
    for K in ([64, 128, 192, 256, 320] if ring4 else [64, 128, 192]):      # prologue depth, first wrap of the ring
        _exact(_run(lib, Problem(m1, BN + 4, K, seed=hint), hint), '%s K=%d' % (name, K))
        _exact(_run(lib, Problem(m1, BN + 4, K, seed=hint), hint, f32=False, bias=False), '%s K=%d bf16 no bias' % (name, K))
    # 3 x 3 = 9 and 3 x 5 = 15 tiles for the hinted forms (more for the auto forms' larger M): tile counts that are no multiple of
    # 8, on either side of the XCD remap's remainder branch
    m3 = Ms[4]
    _exact(_run(lib, Problem(m3, 2 * BN + 4, 128, seed=hint), hint, f32=False), '%s 9 tiles' % name)
    _exact(_run(lib, Problem(m3, 4 * BN + 4, 128, seed=hint), hint), '%s 15 tiles' % name)
    _variants(lib, Problem(m1, BN + 4, 192, seed=hint), hint, name)
    if Ms[0] <= 23 or hint != 0:
        _rowmaps(lib, hint, name)
    else:                                               # auto forms above M = 23: the same map over more groups
        _rowmaps(lib, hint, name, maps=((m1, ROWMAP),))
    Pf = Problem(m1, BN + 4, 192, seed=hint, full=True)
    _close_full(_run(lib, Pf, hint, f32=True, res='sep', pads=STRIDES), 192, 'full-mantissa %s fp32+bias+residual' % name)
    _close_full(_run(lib, Pf, hint, f32=False, pads=STRIDES), 192, 'full-mantissa %s bf16+bias' % name)


def test_auto_picks_128x128_tiles(lib):
    """tile_hint 0 at 256 < M < 2048: the cost model goes to 128x128 tiles once the 64x64 grid passes ~730 tiles (2047 x 1536: 768
    against 192 tiles), and tanh always runs there"""
    P = Problem(2047, 1536, 128, seed=2)
    _exact(_run(lib, P, 0), 'auto 2047x1536x128 fp32+bias')
    _exact(_run(lib, P, 0, f32=False, pads=(8, 8, 4, 0)), 'auto 2047x1536x128 bf16 strided')
    _close_act(_run(lib, Problem(321, 68, 192, seed=2), 0, f32=True, act=ACT_TANH), 'auto 321x68 tanh fp32')


# ------------------------------------------------------------------------------------------------ b. slab forms
@pytest.mark.parametrize('hint', [20, 21, 22, 23, 24])
def test_slab_forms(lib, hint):
    BM, BN, family = FORMS[hint]
    for M in (1, BM, BM + 1):
        for N in (BN, BN + 4):
            for K in (1536, 2304):
                P = Problem(M, N, K, seed=hint)
                r = _run(lib, P, hint, bias=False, pads=(8, 16, 4, 0), kranges=[(k, k + 768) for k in range(0, K, 768)])
                _exact(r, 'hint %d slabs %dx%dx%d' % (hint, M, N, K))          # every slab against its own k range
                got = r.C[G:G + r.S * M].double().view(r.S, M, r.ldc)[:, :, :N].sum(0)
                assert torch.equal(got, P.acc), 'hint %d: the slab sum is not the whole product' % hint
            P = Problem(M, N, 768, seed=hint)
            if family == 'resident':       # K = 768: a finished output, the epilogues dispatch_resident carries
                _exact(_run(lib, P, hint, f32=False, pads=STRIDES), 'hint %d K=768 bf16' % hint)
                _exact(_run(lib, P, hint, f32=True, pads=STRIDES), 'hint %d K=768 fp32+bias' % hint)
                _exact(_run(lib, P, hint, f32=True, res='sep', pads=STRIDES), 'hint %d K=768 fp32+residual' % hint)
                _exact(_run(lib, P, hint, f32=True, res='inplace'), 'hint %d K=768 fp32+residual in place' % hint)
                _close_act(_run(lib, P, hint, f32=False, act=ACT_GELU, pads=STRIDES), 'resident bf16+gelu')
                _close_act(_run(lib, P, hint, f32=True, act=ACT_GELU, pads=STRIDES), 'resident fp32+gelu')
            else:
                _refused(_run(lib, P, hint, bias=False), 'hint %d at K = 768' % hint)
    # what a slab launch cannot carry is refused, and C keeps the sentinel
    P = Problem(BM + 1, BN + 4, 1536, seed=hint)
    kr = [(0, 768), (768, 1536)]
    _refused(_run(lib, P, hint, bias=True, kranges=kr), 'hint %d slabs + bias' % hint)
    _refused(_run(lib, P, hint, bias=False, res='sep', kranges=kr), 'hint %d slabs + residual' % hint)
    _refused(_run(lib, P, hint, bias=False, f32=False, kranges=kr), 'hint %d slabs + bf16' % hint)
    _refused(_run(lib, P, hint, bias=False, act=ACT_GELU, kranges=kr), 'hint %d slabs + gelu' % hint)
    _refused(_run(lib, Problem(BM + 1, BN + 4, 832, seed=hint), hint, bias=False), 'hint %d at K = 832' % hint)
    Pf = Problem(BM + 1, BN + 4, 1536, seed=hint, full=True)
    _close_full(_run(lib, Pf, hint, bias=False, pads=(8, 16, 4, 0), kranges=kr), 768, 'full-mantissa hint %d slabs' % hint)


# ------------------------------------------------------------------------------------------------ c. skinny and split-K
def test_skinny(lib):
    for M in (1, 64, 65, 129):
        for N in (4, 36, 64, 68):
            for K in (128, 256, 384, 512):         # 1..4 chunks of the two-register-set pipeline
                _exact(_run(lib, Problem(M, N, K, seed=4), 4), 'skinny %dx%dx%d fp32+bias' % (M, N, K))
    for M in (64, 65):
        _variants(lib, Problem(M, 68, 384, seed=4), 4, 'skinny M=%d' % M)
    _refused(_run(lib, Problem(65, 68, 192, seed=4), 4), 'skinny at K = 192')
    _refused(_run(lib, Problem(23, 36, 128, seed=4), 4, res='sep', rowmap=ROWMAP + (0,)), 'skinny with a row map')
    Pf = Problem(65, 68, 384, seed=4, full=True)
    _close_full(_run(lib, Pf, 4, f32=True, res='sep', pads=STRIDES), 384, 'full-mantissa skinny fp32+bias+residual')
    _close_full(_run(lib, Pf, 4, f32=False, pads=STRIDES), 384, 'full-mantissa skinny bf16+bias')


def test_split_k(lib):
    for split, Ks in ((2, (256, 512)), (3, (384, 768))):
        for K in Ks:
            kc = K // split
            kr = [(s * kc, (s + 1) * kc) for s in range(split)]
            for M in (1, 64, 65, 256):
                for N in (36, 68):
                    _exact(_run(lib, Problem(M, N, K, seed=split), 0, bias=False, split_k=split, kranges=kr, pads=(8, 16, 4, 0)),
                           'skinny split_k=%d %dx%dx%d' % (split, M, N, K))
    _refused(_run(lib, Problem(65, 68, 320, seed=4), 0, bias=False, split_k=2, kranges=[(0, 160), (160, 320)]), 'K = 320 in two splits')
    _refused(_run(lib, Problem(65, 68, 256, seed=4), 0, bias=False, f32=False, split_k=2, kranges=[(0, 128), (128, 256)]), 'bf16 split-K slabs')
    # 128x128 ragged split: 12 k-tiles over 5 splits of 3 -> the last split owns none and must write zeros
    kr = [(0, 192), (192, 384), (384, 576), (576, 768), (768, 768)]
    for N in (132, 260):
        P = Problem(257, N, 768, seed=5)
        r = _run(lib, P, 0, bias=False, split_k=5, kranges=kr, pads=(8, 16, 4, 0))
        _exact(r, 'ragged split_k=5 257x%dx768' % N)
        assert not bool(r.ref[4].any())                     # (the reference of an empty range is zero)
    Pf = Problem(257, 132, 768, seed=5, full=True)
    _close_full(_run(lib, Pf, 0, bias=False, split_k=5, kranges=kr), 192, 'full-mantissa ragged split-K')
    Pf = Problem(65, 68, 512, seed=5, full=True)
    _close_full(_run(lib, Pf, 0, bias=False, split_k=2, kranges=[(0, 256), (256, 512)]), 256, 'full-mantissa skinny split-K')


# ------------------------------------------------------------------------------------------------ d / e. the 256-column kernels
N256 = [4, 8, 16, 252, 256, 260, 264, 272, 516]       # N % 16, N % 8 and N % 4 on both sides of a 256-column tile


def _sweep_256(lib, hint, BM, Ks, what, m_sweep=257):
    for M in _edges(BM):                              # M edges x the column edge, fp32 + bias
        for N in (252, 256, 260):
            _exact(_run(lib, Problem(M, N, Ks[1], seed=hint), hint), '%s %dx%dx%d fp32+bias' % (what, M, N, Ks[1]))
    for K in Ks:                                      # k loop: 1 / 2 / 3 / 4 .. k-tiles (the `more` / `more2` branches)
        _exact(_run(lib, Problem(m_sweep, 260, K, seed=hint), hint), '%s K=%d fp32+bias' % (what, K))
        _exact(_run(lib, Problem(m_sweep, 264, K, seed=hint), hint, f32=False, pads=(8, 16, 8, 0)), '%s K=%d bf16' % (what, K))
        _exact(_run(lib, Problem(BM + 1, 256, K, seed=hint), hint, f32=False), '%s K=%d bf16 N=256' % (what, K))


def _n_sweep_256(lib, hint, M, K, what):
    """the N sweep with every epilogue variant; the bf16 ones with ldc = N + 8 (16-byte rows) and ldc = N + 4 (8-byte rows)"""
    for N in N256:
        P = Problem(M, N, K, seed=hint)
        for pc in (8, 4):
            pads = (8, 16, pc, 12)
            _exact(_run(lib, P, hint, f32=False, pads=pads), '%s N=%d ldc=N+%d bf16' % (what, N, pc))
            _close_act(_run(lib, P, hint, f32=False, act=ACT_GELU, pads=pads), '%s bf16+gelu' % what)
            _exact(_run(lib, P, hint, f32=False, res='sep', pads=pads), '%s N=%d ldc=N+%d bf16+residual' % (what, N, pc))
        _exact(_run(lib, P, hint, f32=True, pads=(8, 16, 4, 0)), '%s N=%d fp32+bias' % (what, N))
        _exact(_run(lib, P, hint, f32=True, res='inplace', pads=(8, 16, 4, 0)), '%s N=%d fp32+residual in place' % (what, N))
        _close_act(_run(lib, P, hint, f32=True, act=ACT_GELU, pads=(8, 16, 4, 0)), '%s fp32+gelu' % what)


WAVE8 = [(32, 256), (31, 128), (30, 192), (33, 256), (5, 256)]


@pytest.mark.parametrize('hint,BM', WAVE8, ids=['h%d' % h for h, _ in WAVE8])
def test_8wave_shapes(lib, hint, BM):
    _sweep_256(lib, hint, BM, [64, 128, 192, 256], '8-wave hint %d' % hint)
    _rowmaps(lib, hint, '8-wave hint %d' % hint, maps=((23, ROWMAP), (513, (300, 302, 1))), N=260, K=128)
    _refused(_run(lib, Problem(65, 68, 128, seed=hint), hint, act=ACT_TANH), 'tanh under hint %d' % hint)
    Pf = Problem(257, 260, 192, seed=hint, full=True)
    _close_full(_run(lib, Pf, hint, f32=True, res='sep', pads=STRIDES), 192, 'full-mantissa 8-wave hint %d fp32+bias+residual' % hint)
    _close_full(_run(lib, Pf, hint, f32=False, pads=STRIDES), 192, 'full-mantissa 8-wave hint %d bf16+bias' % hint)


@pytest.mark.parametrize('hint,BM', WAVE8, ids=['h%d' % h for h, _ in WAVE8])
def test_8wave_epilogues(lib, hint, BM):
    _n_sweep_256(lib, hint, 257, 128, '8-wave hint %d' % hint)


@pytest.mark.parametrize('hint', [32, 5, 42, 41, 40])
def test_256_column_groups(lib, hint):
    """11 column tiles: groups of 3, 3, 3 and 2, every other group walked backwards"""
    P = Problem(513, 2564, 128, seed=hint)
    _exact(_run(lib, P, hint, f32=True, pads=(8, 16, 4, 0)), 'hint %d 513x2564 fp32+bias' % hint)
    _exact(_run(lib, P, hint, f32=False, pads=(8, 16, 4, 0)), 'hint %d 513x2564 bf16' % hint)
    _exact(_run(lib, Problem(513, 2568, 192, seed=hint), hint, f32=False, pads=(8, 16, 8, 0)), 'hint %d 513x2568 bf16 16-byte rows' % hint)


def _extras(lib, P, hint, what):
    """training extras: aux (the output is (A W^T + bias) * aux), zout (gelu' of the pre-activation) and colsum (+= the column sums of
    the STORED bf16 output)"""
    M, N = P.M, P.N
    r = _run(lib, P, hint, f32=False, aux=True, colsum=True, pads=(8, 16, 8, 0))
    _close_act(r, what + ' aux product')
    assert bool((r.colsum[:4].view(torch.int32) == SENT32).all() and (r.colsum[4 + N:].view(torch.int32) == SENT32).all())
    stored = r.C[G:G + M, :N].double()
    want = r.cs0 + stored.sum(0)
    _measure(what + ' colsum', (r.colsum[4:4 + N].double() - want).abs(), (M + 1) * 2.0 ** -24 * (r.cs0.abs() + stored.abs().sum(0)))
    r = _run(lib, P, hint, f32=False, act=ACT_GELU, zout=True, colsum=True, pads=(8, 16, 8, 0))
    _close_act(r, what + ' gelu with zout')
    zmask = torch.zeros(r.Z.shape, dtype=torch.bool)
    zmask[1:1 + M, :N] = True
    assert bool((r.Z.view(torch.int16)[~zmask] == SENT16).all()), what + ': zout written outside its region'
    zref = _gelu_grad(r.pre)
    _within(what + ' zout', r.Z[1:1 + M, :N], zref, _act_delta(zref), False)
    stored = r.C[G:G + M, :N].double()
    _measure(what + ' colsum', (r.colsum[4:4 + N].double() - (r.cs0 + stored.sum(0))).abs(),
             (M + 1) * 2.0 ** -24 * (r.cs0.abs() + stored.abs().sum(0)))


@pytest.mark.parametrize('hint', [0, 5, 32])
def test_8wave_training_extras(lib, hint):
    for (M, N, K) in ((2049, 264, 128), (2049, 256, 192)):
        _extras(lib, Problem(M, N, K, seed=hint), hint, '8-wave extras')
    # aux / zout on 8-byte rows (the general LDS path), without colsum (which needs 16-byte rows)
    P = Problem(2049, 260, 128, seed=hint)
    _close_act(_run(lib, P, hint, f32=False, aux=True, pads=(8, 16, 4, 0)), '8-wave extras aux product')
    r = _run(lib, P, hint, f32=False, act=ACT_GELU, zout=True, pads=(8, 16, 4, 0))
    _close_act(r, '8-wave extras gelu with zout')
    _within('8-wave extras zout', r.Z[1:2050, :260], _gelu_grad(r.pre), _act_delta(_gelu_grad(r.pre)), False)
    _refused(_run(lib, P, hint, f32=False, colsum=True, pads=(8, 16, 4, 0)), 'colsum with N % 8 != 0')


WAVE4_K = [128, 192, 256, 320, 384, 448]


@pytest.mark.parametrize('hint', [40, 41, 42])
def test_4wave_shapes(lib, hint):
    _sweep_256(lib, hint, 256, WAVE4_K, '4-wave hint %d' % hint)
    _rowmaps(lib, hint, '4-wave hint %d' % hint, maps=((23, ROWMAP), (513, (300, 302, 1))), N=260, K=128)
    _rowmaps(lib, hint, '4-wave hint %d N=256' % hint, maps=((513, (300, 302, 1)),), N=256, K=192)
    _refused(_run(lib, Problem(257, 256, 64, seed=hint), hint), 'K = 64 under hint %d' % hint)
    _refused(_run(lib, Problem(257, 256, 128, seed=hint), hint, act=ACT_TANH), 'tanh under hint %d' % hint)
    Pf = Problem(257, 260, 192, seed=hint, full=True)
    _close_full(_run(lib, Pf, hint, f32=True, res='sep', pads=STRIDES), 192, 'full-mantissa 4-wave hint %d fp32+bias+residual' % hint)
    _close_full(_run(lib, Pf, hint, f32=False, pads=STRIDES), 192, 'full-mantissa 4-wave hint %d bf16+bias' % hint)
    Pf = Problem(513, 512, 448, seed=hint, full=True)
    _close_full(_run(lib, Pf, hint, f32=False), 448, 'full-mantissa 4-wave hint %d bf16+bias 513x512x448' % hint)


@pytest.mark.parametrize('hint', [40, 41, 42])
def test_4wave_epilogues(lib, hint):
    _n_sweep_256(lib, hint, 257, 192, '4-wave hint %d' % hint)


def _took(r, family, what, **fields):
    """the launch went to `family` (vitcap_gemm_plan, asked with the launch's own descriptor) with these plan fields"""
    assert r.rc == 0, '%s refused: %s' % (what, r.err)
    got = dict((k, getattr(r.plan, k)) for k in fields)
    assert (r.family, got) == (family, fields), '%s: planned %s %s, expected %s %s' % (what, r.family, got, family, fields)


@pytest.mark.parametrize('hint', [0, 5])
def test_large_m_forms_and_downgrades(lib, hint):
    """What tile_hint 0 and 5 launch at M = 2049, exact against the reference, with the kernel family of every launch asserted through
    vitcap_gemm_plan.
    hint 0: the auto cost model sits in front of the large-tile family.  For K <= 768 it prices 64x64 tiles at 4 + 0.0165 T64 (T64 =
    33 ceil(N / 64) tiles here), 128x128 tiles at no less than 16 and 256x256 tiles at 23 per round, so every N of this test (<= 516:
    T64 <= 297, 8.9) runs the 64x64 ring -- NOT the 4-wave kernel.  (The 4-wave downgrades 42 -> 41 -> 40 are covered numerically under
    their own hints by test_4wave_shapes / test_4wave_epilogues and test_4wave_downgrades_the_old_queries_cannot_see.)
    hint 5: the 4-wave one-tile form for bf16 outputs without residual from K = 128 on -- register epilogue (form 1) where N and ldc
    are multiples of 8, LDS epilogue (form 0) otherwise -- and the 8-wave kernel for the rest.
    vitcap_gemm_large_form answers for the large-tile family alone (what hint 0 would pick if its cost model got that far); its
    answers are asserted as they always were."""
    M = 2049
    q = lambda N, K, plain=False: lib.vitcap_gemm_large_form(M, N, K, hint | (0x100 if plain else 0))
    if hint == 0:
        assert q(256, 192) % 10 == 2 and q(512, 448) % 10 == 2
        assert q(256, 128) % 10 == 1 and q(264, 192) % 10 == 1 and q(8, 192) % 10 == 1      # 42 -> 41
        assert q(260, 192) % 10 == 0 and q(252, 128) % 10 == 0 and q(4, 192) % 10 == 0      # 42 / 41 -> 40
        assert q(256, 64) == -1                                                             # K < 128: the 8-wave kernel
    else:
        assert q(256, 192) == -1 and q(256, 192, True) % 10 == 1 and q(260, 192, True) % 10 == 0 and q(256, 64, True) == -1

    def took(r, N, K, ldc, plain, what):
        if hint == 0:
            _took(r, 'ring', what, wm=2, wn=2, stages=4, block=256, lds_bytes=4 * 128 * 128, tiles_m=33, tiles_n=(N + 63) // 64)
            assert (r.plan.grid[0], r.plan.grid[1]) == (33 * ((N + 63) // 64), 1)
        elif plain and K >= 128:
            _took(r, '4wave_tile', what, form=1 if N % 8 == 0 and ldc % 8 == 0 else 0, tiles_n=(N + 255) // 256, block=256)
        else:
            _took(r, '8wave', what, ph=4, mts=0, tiles_m=9, tiles_m_small=0, tiles_n=(N + 255) // 256, block=512)

    for K in (64, 128, 192, 448):
        for N in N256:
            P = Problem(M, N, K, seed=hint)
            r = _run(lib, P, hint, f32=False, pads=(8, 16, 8, 0))
            _exact(r, 'hint %d M=2049 N=%d K=%d bf16' % (hint, N, K))
            took(r, N, K, N + 8, True, 'hint %d N=%d K=%d bf16' % (hint, N, K))
            r = _run(lib, P, hint, f32=True, res='inplace', pads=(8, 16, 4, 0))
            _exact(r, 'hint %d M=2049 N=%d K=%d fp32+residual' % (hint, N, K))
            took(r, N, K, N + 4, False, 'hint %d N=%d K=%d fp32+residual' % (hint, N, K))
        for N in (252, 256, 264):
            P = Problem(M, N, K, seed=hint)
            r = _run(lib, P, hint, f32=False, pads=(8, 16, 4, 0))
            _exact(r, 'hint %d M=2049 N=%d K=%d bf16 8-byte rows' % (hint, N, K))
            took(r, N, K, N + 4, True, 'hint %d N=%d K=%d bf16 8-byte rows' % (hint, N, K))
            r = _run(lib, P, hint, f32=False, act=ACT_GELU, pads=(8, 16, 8, 0))
            _close_act(r, 'large-M bf16+gelu')
            took(r, N, K, N + 8, True, 'hint %d N=%d K=%d bf16+gelu' % (hint, N, K))
            r = _run(lib, P, hint, f32=True, pads=(8, 16, 4, 0))
            _exact(r, 'hint %d M=2049 N=%d K=%d fp32+bias' % (hint, N, K))
            took(r, N, K, N + 4, False, 'hint %d N=%d K=%d fp32+bias' % (hint, N, K))
            r = _run(lib, P, hint, f32=False, res='sep', pads=(8, 16, 8, 12))
            _exact(r, 'hint %d M=2049 N=%d K=%d bf16+residual' % (hint, N, K))
            took(r, N, K, N + 8, False, 'hint %d N=%d K=%d bf16+residual' % (hint, N, K))


def test_4wave_downgrades_the_old_queries_cannot_see(lib):
    """Two 4-wave choices that vitcap_gemm_large_form cannot report (it takes no ldc and answers -1 below 2048 rows), asserted through
    vitcap_gemm_plan and exact against the reference.
    (a) bf16 rows that are not 16-byte multiples (ldc = N + 4): the register epilogue's 16-byte stores do not apply, so tile_hint 41 and
        42 both run the one-tile form with the LDS epilogue (form 0: 256-row tiles, MI = 8).
    (b) tile_hint 42 below 2048 rows: 256 columns are one column tile, so M rows are ceil(M / (32 MI)) tiles -- one round of the GPU's
        CUs whatever MI in {8, 7, 6} -- and a round costs 0.3 + MI, so the 192-row tile (MI = 6) wins: two tiles for 193, 225 and 257
        rows, on a grid of two workgroups.  K = 192 is three k-tiles, fewer than the MI / 2 + 3 = 6 the deferred-store variant needs:
        the plain persistent kernel runs."""
    for hint in (41, 42):
        P = Problem(2049, 256, 192, seed=hint)
        r = _run(lib, P, hint, f32=False, pads=(8, 16, 4, 0))
        _exact(r, 'hint %d 2049x256x192 bf16 ldc = N + 4' % hint)
        _took(r, '4wave_tile', 'hint %d ldc = N + 4' % hint, form=0, mi=8, tiles_m=9, tiles_n=1, block=256)
        assert r.plan.grid[0] == 9
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for M in (193, 225, 257):
        # pick_mi's rule, restated: cost = rounds x (0.3 + MI), MI from 8 down, a shorter tile must win 1.5 %
        best, best_c = 8, 1e30
        for mi in (8, 7, 6):
            c = -(-(-(-M // (32 * mi))) // cus) * (0.3 + mi)
            if c < best_c * 0.985:
                best, best_c = mi, c
        assert cus < 2 or best == 6                # one round for every height on any GPU with 2+ CUs: the 192-row tile
        P = Problem(M, 256, 192, seed=M)
        r = _run(lib, P, 42, f32=False, pads=(8, 16, 8, 0))
        _exact(r, 'hint 42 %dx256x192 bf16' % M)
        tiles = -(-M // (32 * best))
        _took(r, '4wave_persistent', 'hint 42 M=%d' % M, form=2, mi=best, variant=0, tiles_m=tiles, tiles_n=1, n_big=tiles, block=256)
        assert r.plan.grid[0] == tiles


class _Reserved(object):
    """vitcap_gemm_reserve_cus so that the persistent grid keeps 8 workgroups; the previous value is restored and checked"""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert cus >= 16 and cus % 8 == 0
        self.prev = self.lib.vitcap_gemm_reserve_cus(cus - 8)
        return self

    def __exit__(self, *exc):
        self.lib.vitcap_gemm_reserve_cus(self.prev)
        assert self.lib.vitcap_gemm_reserve_cus(self.prev) == self.prev == 0


@pytest.mark.parametrize('M,N', [(769, 768), (513, 3072)], ids=['12tiles', '36tiles'])
def test_persistent_several_tiles_per_workgroup(lib, monkeypatch, M, N):
    """tile_hint 42 on an 8-workgroup grid: 12 tiles (some workgroups run two, some one) and 36 tiles in column groups of 3"""
    try:
        with _Reserved(lib):
            for K in (192, 256, 448, 512):              # 448 and 512 are long enough for the deferred stores (K / 64 >= 7)
                P = Problem(M, N, K, seed=42)
                for defer in ('0', '1', '2'):
                    monkeypatch.setenv('VITCAP_GEMM_4W_DEFER', defer)
                    _exact(_run(lib, P, 42, f32=False, pads=(8, 16, 8, 0)), 'persistent %dx%dx%d bf16 defer=%s' % (M, N, K, defer))
                    _close_act(_run(lib, P, 42, f32=False, act=ACT_GELU), 'persistent bf16+gelu')
                monkeypatch.delenv('VITCAP_GEMM_4W_DEFER')
                _exact(_run(lib, P, 42, f32=True, pads=(8, 16, 4, 0)), 'persistent %dx%dx%d fp32+bias' % (M, N, K))
                _exact(_run(lib, P, 42, f32=True, res='inplace'), 'persistent %dx%dx%d fp32+residual' % (M, N, K))
                _exact(_run(lib, P, 42, f32=False, res='sep', pads=(8, 16, 8, 12)), 'persistent %dx%dx%d bf16+residual' % (M, N, K))
    finally:
        assert lib.vitcap_gemm_reserve_cus(0) == 0


def test_persistent_extras_and_tile_heights(lib):
    """on the 8-workgroup grid: the training extras at M = 2049, N = 256, and one M per tile height (256 / 224 / 192 rows) found
    with the host-side query, each with two tiles per workgroup"""
    try:
        with _Reserved(lib):
            for K in (192, 256, 448, 512):
                assert lib.vitcap_gemm_large_form(2049, 256, K, 0) % 10 == 2
                _extras(lib, Problem(2049, 256, K, seed=42), 42, 'persistent extras')
            found = {}
            for M in range(2049, 4097, 2):
                found.setdefault(lib.vitcap_gemm_large_form(M, 256, 192, 0), M)
            assert {82, 72, 62} <= set(found), found
            for code in (82, 72, 62):
                M = found[code]
                tiles = -(-M // (32 * (code // 10)))
                assert 8 < tiles <= 16
                for K in (192, 448):
                    assert lib.vitcap_gemm_large_form(M, 256, K, 0) == code
                    P = Problem(M, 256, K, seed=code)
                    _exact(_run(lib, P, 42, f32=False, pads=(8, 16, 8, 0)), 'persistent height %d M=%d K=%d bf16' % (code // 10, M, K))
                    _exact(_run(lib, P, 42, f32=True, res='inplace'), 'persistent height %d M=%d K=%d fp32+residual' % (code // 10, M, K))
                    _close_act(_run(lib, P, 42, f32=False, act=ACT_GELU), 'persistent bf16+gelu')
    finally:
        assert lib.vitcap_gemm_reserve_cus(0) == 0


def test_persistent_prefetch_form(lib, monkeypatch):
    """The A-panel prefetch form: M >= 65536, 256-row tiles, default defer policy (which does not defer from 64k rows on).  Exact
    against the reference on the 8-workgroup grid, and the full grid gives the same bits."""
    monkeypatch.delenv('VITCAP_GEMM_4W_DEFER', raising=False)
    try:
        with _Reserved(lib):
            M = next(m for m in range(65537, 65537 + 4096, 2) if lib.vitcap_gemm_large_form(m, 256, 192, 0) == 82)
            small = {}
            for K in (192, 256):
                assert lib.vitcap_gemm_large_form(M, 256, K, 0) == 82
                P = Problem(M, 256, K, seed=82)
                r = _run(lib, P, 42, f32=False, pads=(8, 16, 8, 0))
                _exact(r, 'prefetch form %dx256x%d' % (M, K))
                small[K] = (P, r.C)
        P, c8 = small[192]
        r = _run(lib, P, 42, f32=False, pads=(8, 16, 8, 0))
        assert r.rc == 0 and torch.equal(r.C.view(torch.int16), c8.view(torch.int16)), 'full grid and 8-workgroup grid differ'
    finally:
        assert lib.vitcap_gemm_reserve_cus(0) == 0


def test_persistent_grid_size_never_changes_a_bit(lib):
    """full-mantissa operands, persistent form: the full grid and the 8-workgroup grid agree bit for bit (what the training engine
    relies on while a collective holds reserved CUs)"""
    cases = [(769, 768, 448, dict(f32=False)), (513, 3072, 192, dict(f32=False, act=ACT_GELU)), (2049, 256, 256, dict(f32=True, res='sep'))]
    full = []
    for (M, N, K, kw) in cases:
        P = Problem(M, N, K, seed=9, full=True)
        state = P.g.get_state()                        # the second launch draws the same residual values
        r = _run(lib, P, 42, **kw)
        if not kw.get('act'):
            _close_full(r, K, 'full-mantissa persistent %s' % ('fp32+bias+residual' if kw.get('res') else 'bf16+bias'))
        full.append((P, state, r.C))
    try:
        with _Reserved(lib):
            for (P, state, c), (M, N, K, kw) in zip(full, cases):
                P.g.set_state(state)
                r = _run(lib, P, 42, **kw)
                bits = torch.int32 if r.f32 else torch.int16
                assert r.rc == 0 and torch.equal(r.C.view(bits), c.view(bits)), '%dx%dx%d: the reduced grid changed a result bit' % (M, N, K)
    finally:
        assert lib.vitcap_gemm_reserve_cus(0) == 0


# ------------------------------------------------------------------------------------------------ f. row statistics
@pytest.mark.parametrize('M', [1, 65, 256, 257])
def test_rowstat(lib, ops, M):
    """M <= 256: the 64x64 form, 257: the 128x128 form.  Per row and 32-column piece {max, argmax (lowest column on ties), sum exp(x - max)}
    of the exact logits; the lattice produces many ties, which is the point"""
    from vitcap_amd._lib import GemmDesc
    ties = 0
    for N in (4, 36, 64, 100, 132):
        P = Problem(M, N, 128, seed=77)
        logits = P.acc + P.bias
        pieces = 2 * ((N + 63) // 64)
        abuf, aptr = P.dev_operand('A', 136)
        wbuf, wptr = P.dev_operand('W', 144)
        bbuf, bptr = _dev_vec(P.bias)
        cbuf = _sent(M + 2, N + 4, True)
        rs = _sent(1, (M * pieces + 2 * pieces) * 4, True).flatten()
        d = GemmDesc(M=M, N=N, K=128, lda=136, ldw=144, ldc=N + 4, act=0, out_dtype=1, rowstat=rs.data_ptr() + pieces * 16)
        rc = lib.vitcap_gemm_bias_act(C.c_void_p(aptr), C.c_void_p(wptr), C.c_void_p(bptr), None, C.c_void_p(cbuf.data_ptr() + (N + 4) * 4),
                                      C.byref(d), _s())
        assert rc == 0, lib.vitcap_last_error()
        torch.cuda.synchronize()
        exp = _sent(M + 2, N + 4, True, device='cpu')
        exp[1:1 + M, :N] = logits.float()
        assert torch.equal(cbuf.cpu(), exp), 'rowstat %dx%d: logits' % (M, N)
        rs = rs.cpu().view(M + 2, pieces, 4)
        assert bool((rs[0].view(torch.int32) == SENT32).all() and (rs[-1].view(torch.int32) == SENT32).all()), 'piece slots outside [M][pieces] written'
        got = rs[1:1 + M]
        for pc in range(pieces):
            c0, c1 = pc * 32, min(pc * 32 + 32, N)
            if c0 >= N:            # a piece with no valid column can never win, and adds nothing
                assert bool((got[:, pc, 0] == -math.inf).all() and (got[:, pc, 2] == 0).all())
                continue
            x = logits[:, c0:c1]
            mx = x.max(1).values
            first = (x == mx[:, None]).int().argmax(1) + c0           # lowest column among the ties
            assert torch.equal(got[:, pc, 0], mx.float()), 'rowstat %dx%d piece %d: max' % (M, N, pc)
            assert torch.equal(got[:, pc, 1].view(torch.int32).long(), first), 'rowstat %dx%d piece %d: argmax (lowest column on ties)' % (M, N, pc)
            ties += int(((x == mx[:, None]).sum(1) > 1).sum())
            se = torch.exp(x - mx[:, None]).sum(1)
            _measure('rowstat sum exp', (got[:, pc, 2].double() - se).abs(), (c1 - c0) * 2.0 ** -23 * se)
    assert ties > 0 or M == 1, 'no ties: the lowest-column rule was not exercised'
    # the wrapper the decode loop uses gives the same statistics
    P = Problem(M, 132, 128, seed=77)
    out, rs2 = ops.gemm_rowstat(P.A.to(torch.bfloat16).cuda(), P.W.to(torch.bfloat16).cuda(), P.bias.float().cuda())
    assert torch.equal(out.cpu().double(), P.acc + P.bias)
    assert torch.equal(rs2.cpu()[:, :5, :2].view(torch.int32), got[:, :5, :2].view(torch.int32))


# ------------------------------------------------------------------------------------------------ g. live
def test_live_early_exit(lib):
    cases = [(14, 33, 36, 192, {}), (13, 65, 36, 192, {}), (1, 65, 68, 192, {}), (4, 65, 68, 256, {}),
             (23, 65, 36, 1536, dict(bias=False, kranges=[(0, 768), (768, 1536)])),
             (0, 65, 68, 512, dict(bias=False, split_k=2, kranges=[(0, 256), (256, 512)]))]
    for hint, M, N, K, kw in cases:
        P = Problem(M, N, K, seed=hint)
        r = _run(lib, P, hint, live=0, **kw)
        assert r.rc == 0
        bits = r.C.view(torch.int32)
        assert bool((bits == SENT32).all()), 'hint %d: *live == 0, but C was written' % hint
        _exact(_run(lib, P, hint, live=1, **kw), 'hint %d with *live == 1' % hint)
    # M = 2049: `live` is honoured by the small-M kernels only; the launch goes to the 8-wave kernel (vc_4w_supports) and computes
    P = Problem(2049, 260, 192, seed=1)
    _exact(_run(lib, P, 0, f32=False, live=1), 'M = 2049 with *live == 1')
    r = _run(lib, P, 0, f32=False, live=0)
    assert r.rc == 0
    if not bool((r.C.view(torch.int16) == SENT16).all()):      # all or nothing: never a partly written output
        _exact(r, 'M = 2049 with *live == 0')


# ------------------------------------------------------------------------------------------------ h. tile shape never changes a bit
def test_tile_shape_never_changes_a_result_bit(lib, ops):
    """(257, 260, 768) is accepted by every non-slab form; full-mantissa operands, where the claim is not trivial"""
    from vitcap_amd import _lib as L
    P = Problem(257, 260, 768, seed=3, full=True)
    a, w, b = P.A.to(torch.bfloat16).cuda(), P.W.to(torch.bfloat16).cuda(), P.bias.float().cuda()
    x = P.extra(257).float().cuda()
    hints = [h for h, f in FORMS.items() if f[2] != 'ringslab']
    for variant in ('bf16+bias', 'bf16+gelu', 'fp32+residual'):
        outs = {}
        for h in hints:
            if variant == 'bf16+bias':
                outs[h] = ops.gemm_bias_act(a, w, b, tile_hint=h)
            elif variant == 'bf16+gelu':
                outs[h] = ops.gemm_ex(a, w, bias=b, act=L.ACT_GELU_ERF, tile_hint=h)
            else:
                outs[h] = ops.gemm_bias_act(a, w, b, residual=x, out_dtype=torch.float32, tile_hint=h)
        torch.cuda.synchronize()
        ref = P.acc + P.bias
        if variant == 'fp32+residual':
            ref = ref + x.cpu().double()
            mag = P.A.abs() @ P.W.abs().T + P.bias.abs() + x.cpu().double().abs()
            _measure('full-mantissa 257x260x768 fp32+residual', (outs[0].cpu().double() - ref).abs(), 770 * 2.0 ** -23 * mag)
        for h in hints:
            assert torch.equal(outs[h], outs[32]), 'tile_hint %d differs from tile_hint 32 (%s): %d elements' % (
                h, variant, int((outs[h] != outs[32]).sum()))


# ------------------------------------------------------------------------------------------------ i. hint ledger
def test_hint_ledger(lib, ops):
    """vitcap_gemm_ex knows exactly the tile_hint values of FORMS: a new hint without a row in the table fails here"""
    from vitcap_amd._lib import VitcapError
    P = Problem(64, 64, 1536, seed=0)
    a, w = P.A.to(torch.bfloat16).cuda(), P.W.to(torch.bfloat16).cuda()
    accepted = set()
    for h in range(64):
        try:
            ops.gemm_bias_act(a, w, None, out_dtype=torch.float32, tile_hint=h,
                              out=torch.empty((2, 64, 64), device='cuda', dtype=torch.float32))
            accepted.add(h)
        except VitcapError as e:
            if 'unknown tile_hint' not in str(e):
                accepted.add(h)
    torch.cuda.synchronize()
    assert accepted == set(FORMS), sorted(accepted ^ set(FORMS))


def test_print_measured():
    """(last in the file) the largest error / bound ratio per comparison of this session"""
    for k in sorted(MEASURED):
        print('RATIO %-70s %.3g' % (k, MEASURED[k]))
