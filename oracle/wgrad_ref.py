"""References of the weight-gradient GEMM (csrc/gemm_tn.hip: vitcap_gemm_tn, vitcap_gemm_tn_sum) and of its feeders
(vitcap_colsum_bf16, vitcap_transpose_colsum, vitcap_cast_transpose, vitcap_cast_bf16, vitcap_reduce_slabs): exact expected images,
deliberately wrong variants (`mutant=`), inputs and the case tables.  Plain torch on the CPU; nothing here touches the device
library.  Used by tests/test_wgrad_cpu.py and tests/test_hip_wgrad_edges.py; the reasoning is in docs/LAB_tests_wgrad.md.

Most comparisons are EXACT.  The lattice operands (Y integers in -3..3, X integers in -3..3 times 2^-5) make every product and every
partial sum a multiple of 2^-5 below 9 M / 32, which fp32 holds exactly in any order of the additions for every M used here
(M <= 640: below 2^8, 13 significant bits).  So a slab must equal the fp64 product over its own rows bit for bit, and an "image" is
the whole guarded output buffer as it must look after the call: results where the kernel writes, the sentinel everywhere else.
"""
import functools
import math

import torch

SENT32 = 0x7B7B7B7B      # fp32 sentinel (1.3e36, finite: torch.equal sees it)
SENT16 = 0x7B7B          # bf16 sentinel
TB = 256                 # the GEMM's output tile (n and k)
STEP = 64                # rows of one step of a split (the unit `splits` divides)
STAGE = 32               # rows of one ring stage


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def sent_f32(*shape):
    return torch.full(shape, SENT32, dtype=torch.int32).view(torch.float32)


def sent_bf16(*shape):
    return torch.full(shape, SENT16, dtype=torch.int16).view(torch.bfloat16)


# =====================================================================================================================
# operands
# =====================================================================================================================
def _seed(M, N, K, splits):
    return ((M * 4099 + N) * 4099 + K) * 64 + splits


def lattice(M, N, K, splits):
    """Y bf16 [M][N] of integers in -3..3, X bf16 [M][K] of integers in -3..3 times 2^-5, from a generator seeded by the case."""
    g = _gen(_seed(M, N, K, splits))
    Y = torch.randint(-3, 4, (M, N), generator=g).to(torch.bfloat16)
    X = (torch.randint(-3, 4, (M, K), generator=g).to(torch.float32) / 32).to(torch.bfloat16)
    return Y, X


def lattice_preset(N, K, seed):
    """fp32 [N][K] of integers in -64..64 times 2^-5: a preset that keeps the accumulating sums exact."""
    return torch.randint(-64, 65, (N, K), generator=_gen(seed)).to(torch.float32) / 32


def full_mantissa(M, N, K, splits):
    """randn bf16 operands with the planted pair of tests/test_hip_train_ops.py: one hot element that must land at [n][k] = [3][200]."""
    g = _gen(_seed(M, N, K, splits) + 1)
    Y = torch.randn((M, N), generator=g).to(torch.bfloat16)
    X = torch.randn((M, K), generator=g).to(torch.bfloat16)
    Y[7, 3] = 64.0
    X[7, 200] = 32.0
    return Y, X


# =====================================================================================================================
# the split of M (from the header's contract and the launcher: ceil(M / 64) steps, ceil(steps / splits) per split)
# =====================================================================================================================
def split_rows(M, splits, mutant=None):
    """[(begin, end)] per split: rows [s sps 64, min((s + 1) sps 64, M)), (M, M) where the split begins at or behind M."""
    steps = (M + STEP - 1) // STEP
    sps = steps // splits if mutant == 'sps_floor' else (steps + splits - 1) // splits
    out = []
    for s in range(splits):
        a = s * sps * STEP
        b = min((s + 1) * sps * STEP, M)
        out.append((a, b) if a < M and b > a else (min(a, M), min(a, M)))
    return out


def steps_per_split(M, splits):
    return [(b - a + STEP - 1) // STEP for a, b in split_rows(M, splits)]


GEMM_MUTANTS = ('stage_tail', 'step_tail', 'sps_floor', 'empty_unwritten', 'transposed', 'tn_tk_swapped', 'x_rows_4_7',
                'chunk_xor_1', 'split_tile_exchanged')


def slabs_ref(Y, X, splits):
    """fp32 [splits][N][K]: the fp64 product over each split's own rows, cast to fp32; zeros for an empty split."""
    return slab_image(Y, X, splits)[:splits]


def slab_abs_ref(Y, X, splits):
    """(fp64 [splits][N][K] products, fp64 [splits][N][K] products of the absolute values, rows per split)."""
    Yd, Xd = Y.double(), X.double()
    ref, mag, rows = [], [], []
    for a, b in split_rows(Y.shape[0], splits):
        ref.append(Yd[a:b].t() @ Xd[a:b])
        mag.append(Yd[a:b].abs().t() @ Xd[a:b].abs())
        rows.append(b - a)
    return torch.stack(ref), torch.stack(mag), rows


def slab_image(Y, X, splits, mutant=None):
    """The guarded slab buffer after vitcap_gemm_tn: fp32 [splits + 1][N][K], slab s = Y[rows_s]^T X[rows_s], the guard slab untouched.

    Mutants (the errors a kernel of this design can carry; each must differ from the right image on some case of the tables):
      stage_tail            rows >= 32 floor(M / 32) lost (the last partial 32-row stage dropped)
      step_tail             rows >= 64 floor(M / 64) lost (the last partial 64-row step dropped)
      sps_floor             steps per split = floor(steps / splits)
      empty_unwritten       a split without a step leaves its slab as it found it
      transposed            the slab stored as C[k][n]
      tn_tk_swapped         work tile (tn, tk) computes and stores the output tile (tk, tn): tiles beyond the other count never run
      x_rows_4_7            rows 4..7 of each 8-row group of X exchanged with rows 0..3 (the second transpose read), Y untouched
      chunk_xor_1           32-byte chunk c (16 columns) of a Y tile row taken from chunk c ^ 1
      split_tile_exchanged  work item `pos` decoded as tile = pos / tiles, split = pos % tiles
    """
    assert mutant is None or mutant in GEMM_MUTANTS, mutant
    M, N = Y.shape
    K = X.shape[1]
    M8 = (M + 7) // 8 * 8
    Yd = torch.zeros((M8, N), dtype=torch.float64)
    Xd = torch.zeros((M8, K), dtype=torch.float64)
    Yd[:M], Xd[:M] = Y.double(), X.double()
    limit = M8
    if mutant == 'stage_tail':
        limit = M // STAGE * STAGE
    elif mutant == 'step_tail':
        limit = M // STEP * STEP
    elif mutant == 'x_rows_4_7':
        Xd = Xd[torch.arange(M8) ^ 4]
    elif mutant == 'chunk_xor_1':
        Yd = Yd[:, torch.arange(N) ^ 16]
    img = sent_f32(splits + 1, N, K)
    slabs = []
    for s, (a, b) in enumerate(split_rows(M, splits, 'sps_floor' if mutant == 'sps_floor' else None)):
        empty = b <= a
        b = min((b + 7) // 8 * 8, limit)
        slab = (Yd[a:b].t() @ Xd[a:b]) if b > a else torch.zeros((N, K), dtype=torch.float64)
        if mutant == 'transposed':
            slab = slab.t().contiguous().view(N, K)
        slabs.append(slab.float() + 0.0)                # + 0.0: a sum of -0.0 products is +0.0 on an accumulator that starts at +0.0
        if not (empty and mutant == 'empty_unwritten'):
            img[s] = slabs[-1]
    tn_, tk_ = N // TB, K // TB
    if mutant == 'tn_tk_swapped':
        m = min(tn_, tk_)
        out = sent_f32(splits + 1, N, K)
        out[:splits, :m * TB, :m * TB] = img[:splits, :m * TB, :m * TB]
        img = out
    elif mutant == 'split_tile_exchanged':
        tiles = tn_ * tk_
        slabs.append(torch.zeros((N, K)))               # a split index == splits is an empty split writing the guard slab
        out = sent_f32(splits + 1, N, K)
        for pos in range(tiles * splits):
            tile, split = pos // tiles, pos % tiles
            if tile < tiles and split <= splits:        # a tile index beyond the grid stores nothing (n >= N); slabs beyond the guard are not modelled
                n0, k0 = tile // tk_ * TB, tile % tk_ * TB
                out[split, n0:n0 + TB, k0:k0 + TB] = slabs[split][n0:n0 + TB, k0:k0 + TB]
        img = out
    return img


def gemm_bound(mag, rows):
    """|device - fp64| <= (rows + 2) 2^-23 |Y_s|^T |X_s| per element of a slab: the products are exact in fp32, the matrix unit adds
    `rows` of them (zero-page rows add nothing) in an order of its own -- one rounding each at most, counted at one ulp
    (2^-23) instead of half of one for the unit's internal alignment -- plus two for the cast of the reference and the store.  The form
    tests/test_hip_gemm_forms.py uses for its full-mantissa cases."""
    return torch.stack([(r + 2) * 2.0 ** -23 * m for m, r in zip(mag, rows)])


# =====================================================================================================================
# case tables (the CPU file and the GPU file walk the same lists)
# =====================================================================================================================
RING_M = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 321, 640)
CASES_RING = [(M, 256, 512, 1) for M in RING_M]
CASES_TILES = ([(M, N, K, s) for (N, K) in ((256, 256), (512, 256), (256, 512), (512, 768), (768, 512)) for (M, s) in ((129, 1), (300, 3))]
               + [(129, 512, 1024, 1), (300, 512, 1024, 2), (129, 768, 768, 1)])
CASES_SPLITS = [(256, 256, 512, 4), (300, 256, 512, 2), (300, 256, 512, 4), (300, 256, 512, 5), (100, 256, 512, 5), (65, 256, 512, 2),
                (449, 256, 512, 3), (640, 256, 512, 3), (598, 768, 768, 9)]
# (M, N, K, splits, Y buffer width, first column of Y, X buffer width, first column of X): one third of a qkv gradient; the wrappers' call
CASES_STRIDES = [(129, 256, 256, 1, 776, 256, 1040, 512), (300, 256, 256, 2, 776, 256, 1040, 512),
                 (129, 256, 512, 1, 256, 0, 512, 0), (300, 256, 512, 2, 256, 0, 512, 0)]
CASES_FULL = [(129, 256, 512, 1), (300, 512, 768, 3), (640, 256, 256, 3)]
CASES_SUM = [(128, 256, 256, 2), (300, 256, 512, 3), (300, 256, 256, 5), (449, 256, 256, 7), (640, 512, 256, 10), (100, 256, 256, 5)]
SUM_REUSE = (128, 256, 256, 2)
SUM_REUSE_LAUNCHES = 130     # twice round the launcher's 64 ticket slots
SUM_MAX_WORKGROUPS = 20
GEMM_CASES = CASES_RING + CASES_TILES + CASES_SPLITS + [c[:4] for c in CASES_STRIDES]

COLSUM_N = (8, 248, 256, 264, 768)
COLSUM_M = (1, 7, 8, 9, 127, 128, 129, 300)
COLSUM_FULL = (300, 264)
COLSUM_PRESET = 1.5
TRANSPOSE_R = (1, 63, 64, 65, 130)
TRANSPOSE_C = (64, 192)
CT_N = (1, 7, 8, 9, 63, 64, 65, 130)
CT_K = (64, 192)
CAST_N = (4, 1020, 1024, 1028)
REDUCE_S = (1, 2, 5)
REDUCE_N = (4, 1020, 1024, 1028)


def case_id(c):
    return 'M%d-N%d-K%d-s%d' % tuple(c[:4])


def ring_stages(M, splits=1):
    """32-row stages the longest split runs."""
    return 2 * max(steps_per_split(M, splits))


def workgroups(N, K, splits):
    return (N // TB) * (K // TB) * splits


# =====================================================================================================================
# feeders
# =====================================================================================================================
def colsum_lattice(M, N):
    return torch.randint(-3, 4, (M, N), generator=_gen(M * 1031 + N)).to(torch.bfloat16)


def colsum_full(M, N):
    return torch.randn((M, N), generator=_gen(M * 1031 + N + 1)).to(torch.bfloat16)


def colsum_ref(y, preset, mutant=None):
    """fp64 [N]: preset + column sums.  Mutants: 'first_trip' (each 128-row block adds the rows of its first 8-row trip only),
    'col_tail' (columns >= 256 floor(N / 256) not added), 'overwrite' (the preset replaced)."""
    M, N = y.shape
    yd = y.double()
    if mutant == 'first_trip':
        yd = yd[torch.arange(M) % 128 < 8]
    s = yd.sum(0)
    if mutant == 'col_tail':
        s[N // 256 * 256:] = 0
    return s if mutant == 'overwrite' else s + float(preset)


def colsum_bound(y, preset):
    """A thread adds at most 16 rows (128-row block, 8 rows in flight), the block its 8 partials, one atomic per 128-row block."""
    M = y.shape[0]
    return (16 + 8 + math.ceil(M / 128)) * 2.0 ** -24 * (abs(float(preset)) + y.double().abs().sum(0))


def transpose_input(R, C):
    return torch.randint(-3, 4, (R, C), generator=_gen(R * 521 + C)).to(torch.bfloat16)


def ceil_to(v, m):
    return (v + m - 1) // m * m


def transpose_image(x, ldt, guard_rows=2, mutant=None):
    """bf16 [C + guard_rows][ldt] after vitcap_transpose_colsum: xt[c][r] = x[r][c], columns R..ldt zero ('pad_unwritten': left as
    found), the guard rows untouched."""
    R, C = x.shape
    img = sent_bf16(C + guard_rows, ldt)
    if mutant != 'pad_unwritten':
        img[:C] = 0
    img[:C, :R] = x.t()
    return img


def cast_values(n, seed):
    """fp32 [n]: N(0, 1) times 10^U(-3, 3), every third element one of the special values -- rounding midpoints with an even and an odd
    lower neighbour and the values next to them, -0.0, fp32 subnormals, and magnitudes that round to infinity.  No NaN."""
    g = _gen(seed)
    v = torch.randn(n, generator=g) * 10 ** (torch.rand(n, generator=g) * 6 - 3)
    bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,      # 1 + 2^-8 (tie, even below), 1 + 3 2^-8 (tie, odd below), negatives
            0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,      # one ulp either side of both ties
            0x80000000, 0x00000000, 0x00000001, 0x000116C2, 0x80008000, 0x00018000, 0x007FFFFF,   # -0.0, 0.0, subnormals (two of them ties)
            0x7F7F8000, 0x7F7F7FFF, 0xFF7F8000]                  # 3.4e38 -> inf; just below the tie -> largest bf16; -3.4e38 -> -inf
    sp = torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int64).to(torch.int32).view(torch.float32)
    sp = torch.cat([sp, torch.tensor([3.4e38, -3.4e38], dtype=torch.float32)])
    idx = torch.arange(n)
    pick = idx % 3 == 0
    v[pick] = sp[(idx[pick] // 3) % len(sp)]
    assert not bool(torch.isnan(v).any())
    return v


def rne_bf16(x, mutant=None):
    """Round-to-nearest-even fp32 -> bf16 in integer arithmetic on the bits (no NaN handling: the inputs hold none).  'trunc': the low
    half dropped."""
    assert x.dtype == torch.float32
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    if mutant != 'trunc':
        u = u + 0x7FFF + ((u >> 16) & 1)
    r = (u >> 16) & 0xFFFF
    r = torch.where(r >= 0x8000, r - 0x10000, r)
    return r.to(torch.int16).view(torch.bfloat16).view(x.shape)


def cast_transpose_images(w, ldt, mutant=None):
    """(bf16 [N + 1][K], bf16 [K + 1][ldt]) after vitcap_cast_transpose with both outputs: RNE(w) and its transpose, columns N..ldt
    of the transpose and both guard rows untouched.  Mutants: 'trunc'; 'tail_unwritten' (columns >= 8 floor(N / 8) of the transpose,
    the ones stored one by one, left as found)."""
    N, K = w.shape
    wb = rne_bf16(w, 'trunc' if mutant == 'trunc' else None)
    a = sent_bf16(N + 1, K)
    a[:N] = wb
    t = sent_bf16(K + 1, ldt)
    nw = N // 8 * 8 if mutant == 'tail_unwritten' else N
    t[:K, :nw] = wb.t()[:, :nw]
    return a, t


def reduce_values(S, n, seed):
    """fp32 [S][n] spread over four decades (N(0, 1) times 10^U(-2, 2)) and a preset [n]: full mantissas, so the order of the additions
    shows in the bits."""
    g = _gen(seed)
    v = torch.randn((S, n), generator=g) * 10 ** (torch.rand((S, n), generator=g) * 4 - 2)
    return v, torch.randn(n, generator=g)


def reduce_slabs_f32(slabs, out0, accumulate, mutant=None):
    """Bit-exact fp32 emulation of vitcap_reduce_slabs: a = out or 0; a += slab[s] in slab order.  Mutants: 'reverse' (slab order),
    'no_accumulate'."""
    assert slabs.dtype == torch.float32
    a = out0.clone() if accumulate and mutant != 'no_accumulate' else torch.zeros_like(slabs[0])
    order = range(slabs.shape[0] - 1, -1, -1) if mutant == 'reverse' else range(slabs.shape[0])
    for s in order:
        a = a + slabs[s]
    return a


@functools.lru_cache(maxsize=None)
def lattice_case(M, N, K, splits):
    """(Y, X, right image) of a lattice case, computed once per process and shared: treat as read-only."""
    Y, X = lattice(M, N, K, splits)
    return Y, X, slab_image(Y, X, splits)
