"""Teeth of tests/test_hip_wgrad_edges.py, checked without a GPU and without a kernel (docs/LAB_tests_wgrad.md).

The GPU file compares whole guarded output buffers with the expected images of oracle/wgrad_ref.py under torch.equal.  A kernel that
carries an error produces the image of the equally wrong reference, so it is certain to fail wherever that image differs from the
right one in a single element.  This file requires, for every mutant, at least one NAMED case of the GPU file's own tables on which
the two images differ, prints the cases that do, and fails if none does.  It also checks that split_rows partitions [0, M), that the
lattice operands are exact in fp32 in any order, that the fp32 emulations are what they claim, and that plain fp32 arithmetic (torch
on the CPU) stays within the bounds the two full-mantissa comparisons use.
"""
import pytest
import torch

from oracle import wgrad_ref as R


def _killers(name, differs, need=()):
    """differs: {case id: bool}.  Prints the killing cases; at least one is required, and one in each group of `need` (lists of ids)."""
    hit = [c for c, d in differs.items() if d]
    print('TEETH %-24s killed by %d of %d cases: %s' % (name, len(hit), len(differs), ', '.join(hit[:12]) + (' ...' if len(hit) > 12 else '')))
    assert hit, '%s: no case of the tables sees it' % name
    for group in need:
        assert any(differs[c] for c in group), '%s: none of %s sees it' % (name, group)
    return hit


def _differs(a, b):
    return not torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# the GEMM
# ---------------------------------------------------------------------------------------------------------------------
def test_case_tables_are_what_the_note_says():
    assert [R.ring_stages(M) for M in R.RING_M] == [2] * 6 + [4] * 3 + [6] * 3 + [8] * 2 + [10, 12, 20]
    assert all(M % 32 in (0, 1, 31) for M in R.RING_M)
    assert [R.workgroups(N, K, s) for _, N, K, s in R.CASES_TILES] == [1, 3, 2, 6, 2, 6, 6, 18, 6, 18, 8, 16, 9]
    want = {(256, 4): [1, 1, 1, 1], (300, 2): [3, 2], (300, 4): [2, 2, 1, 0], (300, 5): [1] * 5, (100, 5): [1, 1, 0, 0, 0], (65, 2): [1, 1],
            (449, 3): [3, 3, 2], (640, 3): [4, 4, 2], (598, 9): [2] * 5 + [0] * 4}
    for M, N, K, s in R.CASES_SPLITS:
        assert R.steps_per_split(M, s) == want[(M, s)], (M, s)
    assert R.split_rows(65, 2) == [(0, 64), (64, 65)] and R.split_rows(449, 3)[2] == (384, 449) and R.split_rows(300, 2)[1] == (192, 300)
    assert all(R.workgroups(N, K, s) <= R.SUM_MAX_WORKGROUPS for _, N, K, s in R.CASES_SUM)
    assert R.SUM_REUSE_LAUNCHES > 2 * 64


@pytest.mark.parametrize('case', R.GEMM_CASES + R.CASES_FULL + R.CASES_SUM, ids=R.case_id)
def test_split_rows_partition(case):
    M, _, _, splits = case
    rows = R.split_rows(M, splits)
    assert len(rows) == splits
    at = 0
    for a, b in rows:
        assert a <= b
        if b > a:
            assert a == at and a % 64 == 0
            at = b
    assert at == M


def test_lattice_is_exact_in_fp32_in_any_order():
    """fp32 products accumulated forwards, backwards and by torch's own matmul give the fp64 result on the longest case."""
    M, N, K, s = 640, 256, 512, 1
    Y, X, img = R.lattice_case(M, N, K, s)
    assert int(Y.float().abs().max()) == 3 and float(X.float().abs().max()) == 3 / 32
    assert float((Y.float().abs().t() @ X.float().abs()).max()) <= 9 * M / 32 < 2 ** 8
    yf, xf = Y.float(), X.float()
    assert torch.equal(yf.t() @ xf, img[0])
    assert torch.equal(yf.flip(0).t() @ xf.flip(0), img[0])
    acc = torch.zeros(N, K)
    for m in range(M - 1, -1, -1):
        acc += yf[m][:, None] * xf[m][None, :]
    assert torch.equal(acc, img[0])


NEED = {
    'transposed': ([R.case_id(c) for c in R.GEMM_CASES if c[1] == c[2]], [R.case_id(c) for c in R.GEMM_CASES if c[1] != c[2]]),
    'tn_tk_swapped': ([R.case_id(c) for c in R.GEMM_CASES if c[1] != c[2]],),
    'split_tile_exchanged': ([R.case_id(c) for c in R.GEMM_CASES if R.workgroups(c[1], c[2], 1) > 1 and c[3] > 1],),
    'empty_unwritten': ([R.case_id(c) for c in R.CASES_SPLITS if 0 in R.steps_per_split(c[0], c[3])],),
}


@pytest.mark.parametrize('mutant', R.GEMM_MUTANTS)
def test_gemm_mutants_are_seen(mutant):
    differs = {}
    for c in dict.fromkeys(R.GEMM_CASES):
        Y, X, right = R.lattice_case(*c)
        differs[R.case_id(c)] = _differs(R.slab_image(Y, X, c[3], mutant), right)
    hit = _killers('gemm_tn ' + mutant, differs, NEED.get(mutant, ()))
    if mutant == 'stage_tail':          # exactly the cases with a partial last stage
        assert set(hit) == {R.case_id(c) for c in R.GEMM_CASES if c[0] % 32}
    if mutant == 'step_tail':
        assert set(hit) == {R.case_id(c) for c in R.GEMM_CASES if c[0] % 64}
    if mutant == 'tn_tk_swapped':       # invisible where the tile counts agree: the N != K cases are what the tables need them for
        assert not any(differs[R.case_id(c)] for c in R.GEMM_CASES if c[1] == c[2])


@pytest.mark.parametrize('mutant', ['stage_tail', 'sps_floor', 'empty_unwritten'])
def test_sum_cases_see_the_split_mutants(mutant):
    """Section F compares the SUM over the splits: what of the split mutants shows there (sentinels in unwritten slabs add up too)."""
    differs = {}
    for c in R.CASES_SUM:
        Y, X, right = R.lattice_case(*c)
        differs[R.case_id(c)] = _differs(R.slab_image(Y, X, c[3], mutant)[:c[3]].sum(0), right[:c[3]].sum(0))
    _killers('gemm_tn_sum ' + mutant, differs)


@pytest.mark.parametrize('case', R.CASES_FULL, ids=R.case_id)
def test_full_mantissa_bound_has_room(case):
    M, N, K, s = case
    Y, X = R.full_mantissa(*case)
    ref, mag, rows = R.slab_abs_ref(Y, X, s)
    bound = R.gemm_bound(mag, rows)
    got = torch.stack([Y[a:b].float().t() @ X[a:b].float() for a, b in R.split_rows(M, s)]).double()
    ratio = float(((got - ref).abs() / bound).max())
    print('ROOM  gemm_tn %s fp32 arithmetic at %.3f bounds' % (R.case_id(case), ratio))
    assert ratio <= 1.0
    assert float(ref[0][3, 200]) > 2000 and abs(float(ref[0][200, 3])) < 200      # the planted pair lands at [n][k]


# ---------------------------------------------------------------------------------------------------------------------
# the feeders
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mutant', ['first_trip', 'col_tail', 'overwrite'])
def test_colsum_mutants_are_seen(mutant):
    differs = {}
    for N in R.COLSUM_N:
        for M in R.COLSUM_M:
            y = R.colsum_lattice(M, N)
            differs['M%d-N%d' % (M, N)] = _differs(R.colsum_ref(y, R.COLSUM_PRESET, mutant).float(), R.colsum_ref(y, R.COLSUM_PRESET).float())
    hit = _killers('colsum ' + mutant, differs)
    if mutant == 'first_trip':
        assert all(int(h.split('-')[0][1:]) > 8 for h in hit)
    if mutant == 'col_tail':
        assert all(int(h.split('N')[1]) % 256 for h in hit)


def test_colsum_lattice_is_exact_and_bound_has_room():
    y = R.colsum_lattice(300, 768)
    assert torch.equal(y.float().sum(0) + 1.5, R.colsum_ref(y, 1.5).float()) and torch.equal(y.float().flip(0).sum(0) + 1.5, R.colsum_ref(y, 1.5).float())
    y = R.colsum_full(*R.COLSUM_FULL)
    ratio = float(((y.float().sum(0) + 1.5).double() - R.colsum_ref(y, 1.5)).abs().div(R.colsum_bound(y, 1.5)).max())
    print('ROOM  colsum M%d-N%d fp32 arithmetic at %.3f bounds' % (R.COLSUM_FULL + (ratio,)))
    assert ratio <= 1.0


def test_transpose_padding_mutant_is_seen():
    differs = {}
    for Rr in R.TRANSPOSE_R:
        for extra in (0, 64):
            x = R.transpose_input(Rr, 64)
            ldt = R.ceil_to(Rr, 64) + extra
            differs['R%d-ldt%d' % (Rr, ldt)] = _differs(R.transpose_image(x, ldt, mutant='pad_unwritten'), R.transpose_image(x, ldt))
    hit = _killers('transpose pad_unwritten', differs)
    assert 'R64-ldt64' not in hit and 'R64-ldt128' in hit      # at R = 64 only the extra 64 columns are padding


@pytest.mark.parametrize('mutant', ['trunc', 'tail_unwritten'])
def test_cast_transpose_mutants_are_seen(mutant):
    differs = {}
    for N in R.CT_N:
        for K in R.CT_K:
            w = R.cast_values(N * K, N * 131 + K).view(N, K)
            ldt = R.ceil_to(N, 8)
            a, t = R.cast_transpose_images(w, ldt)
            am, tm = R.cast_transpose_images(w, ldt, mutant)
            differs['N%d-K%d' % (N, K)] = _differs(a.view(torch.int16), am.view(torch.int16)) or _differs(t.view(torch.int16), tm.view(torch.int16))
    hit = _killers('cast_transpose ' + mutant, differs)
    if mutant == 'tail_unwritten':
        assert {h.split('-')[0] for h in hit} == {'N%d' % N for N in R.CT_N if N % 8}


def test_rne_emulation_is_torch_and_sees_the_specials():
    for n in R.CAST_N:
        v = R.cast_values(n, 7000 + n)
        assert torch.equal(R.rne_bf16(v).view(torch.int16), v.to(torch.bfloat16).view(torch.int16))
    v = R.cast_values(1028, 8028)
    b = R.rne_bf16(v)
    f = b.float()
    one = torch.tensor([0x3F808000, 0x3F818000], dtype=torch.int32).view(torch.float32)
    assert R.rne_bf16(one).view(torch.int16).tolist() == [0x3F80, 0x3F82]           # ties: to the even neighbour, down and up
    assert bool(torch.isinf(f[v == 3.4e38]).all()) and int((v == torch.tensor(3.4e38)).sum()) > 0
    assert bool(((v == 0) & (v.view(torch.int32) != 0)).any())                      # -0.0 is among them
    assert bool(((v != 0) & (v.abs() < 2.0 ** -126)).any())                         # subnormals too
    assert _differs(R.rne_bf16(v, 'trunc').view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize('mutant', ['reverse', 'no_accumulate'])
def test_reduce_mutants_are_seen(mutant):
    differs = {}
    for S in R.REDUCE_S:
        for n in R.REDUCE_N:
            for acc in (False, True):
                v, pre = R.reduce_values(S, n, S * 10007 + n)
                differs['S%d-n%d-%s' % (S, n, 'acc' if acc else 'plain')] = _differs(R.reduce_slabs_f32(v, pre, acc, mutant), R.reduce_slabs_f32(v, pre, acc))
    hit = _killers('reduce_slabs ' + mutant, differs)
    if mutant == 'reverse':
        assert any(h.startswith('S5') and h.endswith('plain') for h in hit)
    else:
        assert all(h.endswith('acc') for h in hit) and len(hit) == len(differs) // 2


def test_reduce_emulation_is_sequential_fp32():
    v, pre = R.reduce_values(5, 1024, 99)
    want = pre.clone()
    for s in range(5):
        want = (want.double() + v[s].double()).float()      # one fp32 rounding per addition, in slab order
    assert torch.equal(R.reduce_slabs_f32(v, pre, True), want)
    assert torch.equal(R.reduce_slabs_f32(v[:1], pre, False), v[0])
