"""Input side, CPU half (no GPU): the teeth of tests/test_hip_input_side.py.

(1) On the case tables of oracle/input_side_cases.py the project's numpy restatements -- oracle.jpeg_backhalf.backhalf behind the host front
    half, image_oracle.resample_restated + crop, image_oracle.train_transform_restated -- equal Pillow bit for bit, so the tables hold
    nothing the restated rules do not explain.
(2) A restatement with ONE rule changed (the mutants of oracle/input_side_cases.py) is told apart from Pillow by at least one case of its
    table: a device kernel with that rule wrong cannot pass the GPU file, which compares with Pillow on the same cases.
(3) The tables keep the properties they were built for: the B1 geometry conditions, the A2 block layouts, the A7 coefficient bound."""
import numpy as np
import pytest

from oracle import image_oracle as IO
from oracle import input_side_cases as T
from oracle import jpeg_backhalf as JB
from vitcap_amd import jpegdec as J

needs_lib = pytest.mark.skipif(J.jpeg_lib() is None, reason='libvitcap_jpeg.so not built')
_DECODED = {}


def _decoded(key, cases):
    """[(name, parameters, (info, coefs) or None, Pillow's pixels)] of a JPEG table, decoded once per process."""
    if key not in _DECODED:
        _DECODED[key] = [(name, pr, J.decode_coefs(data), T.pillow_rgb(data)) for name, data, pr in cases]
    return _DECODED[key]


def _jpeg_tables():
    out = []
    for mode in T.MODES:
        out += _decoded('a1' + mode, T.a1_cases(mode))
    return out + _decoded('a2', T.a2_cases()) + _decoded('a2x', T.a2x_cases())


# ---------------------------------------------------------------------------------------------------------------- A
@needs_lib
@pytest.mark.parametrize('mode', T.MODES)
def test_a1_front_half_plus_restated_back_half_equals_pillow(mode):
    n = 0
    for name, pr, got, want in _decoded('a1' + mode, T.a1_cases(mode)):
        assert (got is None) == T.front_half_refuses(mode, pr['w']), name          # refused: exactly the streams outside the subset
        if got is None:
            continue
        info, coefs = got
        assert (info.width, info.height, info.ncomp) == (pr['w'], pr['h'], 1 if mode == 'grey' else 3)
        assert np.array_equal(JB.backhalf(info, coefs), want), name
        n += 1
    assert n == (1600 if mode in ('grey', '444') else 1600 - 4 * 40)
    assert {pr['w'] % 16 for _, pr, _, _ in _DECODED['a1' + mode]} == set(range(16)) == {pr['h'] % 16 for _, pr, _, _ in _DECODED['a1' + mode]}


@needs_lib
def test_a2_block_layouts_and_restated_back_half_equals_pillow():
    for name, pr, got, want in _decoded('a2', T.a2_cases()):
        info, coefs = got
        assert int(info.nblocks) == pr['nblocks'], name
        if info.ncomp == 3:
            assert tuple(info.block0) == pr['block0'], name
        assert T.a2_edge_holds(info, pr['edge']), (name, pr['edge'])
        assert np.array_equal(JB.backhalf(info, coefs), want), name
    # A2x is where Pillow's pixels depend on HOW its libjpeg-turbo runs: the SIMD inverse DCT (every ordinary build) saturates samples far
    # out of range, the C path (a build without SIMD, or JSIMD_FORCENONE=1 in the environment) wraps them through its 10-bit table.  The
    # kernel and the restatement follow the SIMD form; on a host of the other kind these cases and the range-limit mutant fail.
    wrap = T.jpeg_mutants()['range limit with the 10-bit wrap of the C path']
    for name, pr, got, want in _decoded('a2x', T.a2x_cases()):
        info, coefs = got
        assert T.idct_fits_int32(info, coefs), name
        assert not np.array_equal(wrap.backhalf(info, coefs), want), "%s: this Pillow's libjpeg-turbo decodes without its SIMD inverse DCT" % name
        assert np.array_equal(JB.backhalf(info, coefs), want), name
        assert (want == 0).any() and (want == 255).any()


@needs_lib
def test_a3_a5_streams_decode():
    for name, data, pr in T.a3_cases()[::16] + T.a5_cases():
        got = J.decode_coefs(data)
        assert got is not None, name
        assert np.array_equal(JB.backhalf(*got), T.pillow_rgb(data)), name


@needs_lib
def test_jpeg_mutants_are_told_apart_from_pillow():
    table = [c for c in _jpeg_tables() if c[2] is not None]
    # the cheapest likely killers first: subsampled modes at odd sizes, then the rest
    table.sort(key=lambda c: (c[1]['mode'] in ('grey', '444'), c[1]['w'] * c[1]['h']))
    for rule, M in T.jpeg_mutants().items():
        killer = next((name for name, pr, (info, coefs), want in table if not np.array_equal(M.backhalf(info, coefs), want)), None)
        print('%-50s killed by %s' % (rule, killer))
        assert killer is not None, 'the JPEG tables cannot see: %s' % rule


def _dequantised_max(info, coefs):
    m = 0
    b0 = [int(v) for v in info.block0] + [int(info.nblocks)]
    for c in range(3 if info.ncomp == 3 else 1):
        qt = np.array(info.qt[c][:], dtype=np.int64)
        lo, hi = b0[c], (b0[c + 1] if info.ncomp == 3 else int(info.nblocks))
        m = max(m, int(np.abs(coefs[lo * 64:hi * 64].astype(np.int64).reshape(-1, 64) * qt).max()))
    return m


@needs_lib
def test_a7_coefficient_bound_and_24_bit_precondition():
    """ENCODER_MAX bounds what Pillow's encoder produces on these tables and on the extreme quality / qtables settings; the synthetic
    coefficients of A7 reach 4x that and still keep every multiply operand of the restated IDCT within +-2^23 (the precondition of the
    kernel's 24-bit multiplies) and every product and sum within int32; the first uniform magnitude that leaves 24 bits lies above."""
    seen = 0
    for name, pr, got, want in _jpeg_tables():
        if got is not None and not name.startswith('a2x'):
            seen = max(seen, _dequantised_max(*got))
    arr, bw = T.synth(70, 50, 3), T.binary(50, 70, 4)
    for img in (arr, bw):
        for kw in (dict(quality=1), dict(quality=2), dict(quality=5), dict(quality=100), dict(qtables=[[1] * 64] * 2),
                   dict(qtables=[[255] * 64] * 2), dict(qtables=[[1 + (37 * i) % 255 for i in range(64)], [255 - (11 * i) % 255 for i in range(64)]])):
            for mode in ('444', '420'):
                got = J.decode_coefs(T.jpeg_stream(img, mode, **kw))
                assert got is not None
                seen = max(seen, _dequantised_max(*got))
    print('largest dequantised magnitude an encoder produced:', seen)
    assert seen <= T.ENCODER_MAX and T.A7_MAGNITUDE == 4 * T.ENCODER_MAX
    worst = 0
    for k, (mode, w, h) in enumerate(T.A7_LAYOUTS):
        info, _ = J.decode_coefs(T.jpeg_stream(T.synth(w, h, k), mode, quality=75))
        coefs = T.a7_coefs(info, 50 + k)
        assert _dequantised_max(info, coefs) <= T.A7_MAGNITUDE and _dequantised_max(info, coefs) > 3 * T.ENCODER_MAX
        worst = max(worst, T.idct_intermediates_max(info, coefs))
        assert T.idct_fits_int32(info, coefs)
    print('largest multiply operand on the A7 inputs: %d (2^23 = %d)' % (worst, 1 << 23))
    assert worst < 1 << 23
    first = first_uniform_magnitude_outside_24_bits()
    print('first uniform magnitude with an operand outside 24 signed bits:', first)
    assert first > T.A7_MAGNITUDE


def first_uniform_magnitude_outside_24_bits():
    """Smallest m such that a block whose 64 dequantised coefficients all have magnitude m (worst of a few sign patterns) gives the
    restated IDCT a multiply operand outside +-2^23."""
    class Info(object):
        ncomp, nblocks, block0, qt = 1, 4, [0, 0, 0], [[1] * 64] * 3
    r, c = np.mgrid[0:8, 0:8]
    signs = np.stack([np.ones((8, 8)), (-1.0) ** r, (-1.0) ** c, (-1.0) ** (r + c)]).astype(np.int64).reshape(4, 64)
    lo, hi = 1, 1 << 22
    while lo < hi:
        m = (lo + hi) // 2
        if T.idct_intermediates_max(Info, (signs * m).reshape(-1)) >= 1 << 23:
            hi = m
        else:
            lo = m + 1
    return lo


# ---------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize('crop,resize_short', T.B1_SETTINGS)
def test_b1_table_conditions(crop, resize_short):
    cases, sub = T.b1_cases(crop, resize_short), T.b1_subset(crop, resize_short)
    assert len(cases) >= 1200 and len(sub) >= 200
    assert T.b1_conditions(cases) == []
    assert T.b1_conditions(sub) == []


@pytest.mark.parametrize('crop,resize_short', T.B1_SETTINGS)
def test_b1_restatement_equals_pillow(crop, resize_short):
    for case in T.b1_subset(crop, resize_short):
        img = T.image_of(case)
        a8, af = IO.transform_reference(img, resize_short, crop)
        b8, bf = T.transform_restated(img, resize_short, crop)
        assert np.array_equal(a8, b8) and np.array_equal(af, bf), case[0]


@pytest.mark.parametrize('resize_short', [384, 426, 438])
def test_b2_restatement_equals_pillow(resize_short):
    firsts = [set(), set()]
    for case in T.b2_cases(resize_short):
        img = T.image_of(case)
        h, w = img.shape[:2]
        nh, nw = IO.resized_size(h, w, resize_short)
        top, left = IO.crop_origin(nh, nw, 384)
        firsts[0].add(T.first_tap(h, nh, top) > 0)
        firsts[1].add(T.first_tap(w, nw, left) > 0)
        a8, af = IO.transform_reference(img, resize_short, 384)
        b8, bf = T.transform_restated(img, resize_short, 384)
        assert np.array_equal(a8, b8) and np.array_equal(af, bf), case[0]
    assert True in firsts[0] and True in firsts[1]         # the window of needed source rows / columns starts past 0 on both axes


def test_resize_mutants_are_told_apart_from_pillow():
    table = [c for s in T.B1_SETTINGS for c in T.b1_subset(*s)]
    table.sort(key=lambda c: c[1][0] * c[1][1])
    refs = {}
    for rule, M in T.resize_mutants().items():
        killer = None
        for case in table:
            pr = case[2]
            if case[0] not in refs:
                refs[case[0]] = IO.transform_reference(T.image_of(case), pr['resize_short'], pr['crop'])[0]
            want = refs[case[0]]
            h, w = case[1][:2]
            nh, nw = M.resized_size(h, w, pr['resize_short'])
            if min(nh, nw) < pr['crop']:
                continue
            got = T.transform_restated(T.image_of(case), pr['resize_short'], pr['crop'], M)[0]
            if got.shape != want.shape or not np.array_equal(got, want):
                killer = case[0]
                break
        print('%-55s killed by %s' % (rule, killer))
        if rule in T.EQUIVALENT_RESIZE_MUTANTS:          # provably the same arithmetic: identical weights for every size of the table
            assert killer is None
            sizes = {(n_in, n_out) for c in table for n_in, n_out in zip(c[1][:2], IO.resized_size(c[1][0], c[1][1], c[2]['resize_short']))}
            assert all(np.array_equal(T.dense_weights(M, a, b), T.dense_weights(IO, a, b)) for a, b in sizes)
            continue
        assert killer is not None, 'the B1 table cannot see: %s' % rule


# ---------------------------------------------------------------------------------------------------------------- C
def _train_cases():
    return T.c1_cases() + T.c2_cases() + T.c3_cases()


_TRAIN_REF = {}


def _train_ref(case):
    if case[0] not in _TRAIN_REF:
        pr = case[2]
        _TRAIN_REF[case[0]] = IO.train_transform_reference(case[1], pr['box'], pr['ops'], pr['flip'], pr['size'])
    return _TRAIN_REF[case[0]]


def test_c_restatement_equals_pillow():
    names = set()
    for case in _train_cases():
        pr = case[2]
        a8, af = _train_ref(case)
        b8, bf = IO.train_transform_restated(case[1], pr['box'], pr['ops'], pr['flip'], pr['size'])
        assert np.array_equal(a8, b8) and np.array_equal(af, bf), case[0]
        names.add(case[0])
    assert len(names) == len(_train_cases())


def test_c3_plants_the_mean_on_the_half():
    for name, img, pr in T.c3_cases():
        L = IO.rgb_to_l(img).astype(np.int64)
        tot, n = int(L.sum()), L.size
        assert 2 * tot in (21 * n, 21 * n - 2), name             # mean exactly 10.5, or one pixel below it
        assert int(tot / n + 0.5) == (11 if 2 * tot == 21 * n else 10)


def test_train_mutants_are_told_apart_from_pillow():
    table = sorted(_train_cases(), key=lambda c: c[2]['size'])
    for rule, M in T.train_mutants().items():
        killer = None
        for case in table:
            pr = case[2]
            if not np.array_equal(M.train_transform_restated(case[1], pr['box'], pr['ops'], pr['flip'], pr['size'])[0], _train_ref(case)[0]):
                killer = case[0]
                break
        print('%-50s killed by %s' % (rule, killer))
        if rule in T.EQUIVALENT_TRAIN_MUTANTS:           # the same arithmetic: the horizontal weight tables are mirror-symmetric
            assert killer is None
            for w, size in sorted({(c[2]['box'][3], c[2]['size']) for c in table}):
                K = T.dense_weights(IO, w, size, 'bilinear')
                assert np.array_equal(K, K[::-1, ::-1]), (w, size)
            continue
        assert killer is not None, 'the train tables cannot see: %s' % rule
