"""TEST INFRASTRUCTURE ONLY (oracle/): the case tables of the input-side parity suites and the mutants that prove the tables have
teeth.  tests/test_input_side_cpu.py (no GPU) and tests/test_hip_input_side.py (MI355X) iterate the SAME tables: the CPU file pins the
numpy restatements (oracle/jpeg_backhalf.py, oracle/image_oracle.py) against Pillow on them and shows that a restatement with one rule
changed is told apart from Pillow by at least one case; the GPU file compares the kernels with Pillow on every case.

Pure Python / numpy / Pillow; the JPEG tables additionally need the host front half (vitcap_amd/libvitcap_jpeg.so) to turn a stream
into (vitcap_jpeg_info, coefficients).  Tables are functions returning lists of (name, payload, parameters); the expensive ones are
cached per process."""
import functools
import inspect
import io
import itertools
import math
import types

import numpy as np
from PIL import Image

from oracle import image_oracle as IO
from oracle import jpeg_backhalf as JB

# ------------------------------------------------------------------------------------------------------------------
# Content
# ------------------------------------------------------------------------------------------------------------------


def synth(w, h, seed):
    """Photo-like content: smooth gradients + texture + hard edges (every AC band and the clamps get exercised)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 100 * np.sin(xx / (7.0 + c) + seed) * np.cos(yy / (11.0 - c)) for c in range(3)], -1)
    img += rng.randn(h, w, 3) * 25
    img[h // 3:h // 2, w // 4:w // 2] = rng.randint(0, 2, 3) * 255
    return np.clip(img, 0, 255).astype(np.uint8)


def jpeg_bytes(arr, **kw):
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format='JPEG', **kw)
    return b.getvalue()


def pillow_rgb(data):
    im = Image.open(io.BytesIO(data))
    return np.asarray(im.convert('RGB') if im.mode != 'RGB' else im)


def smooth(h, w, seed):
    """Low-frequency colour field + noise (the `_img` of tests/test_image_transform_cpu.py)."""
    g = np.random.default_rng(seed)
    base = g.integers(0, 256, size=(h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
    big = np.asarray(Image.fromarray(base, 'RGB').resize((w, h), Image.BILINEAR)).copy()
    noise = g.integers(-20, 21, size=big.shape)
    return np.clip(big.astype(np.int64) + noise, 0, 255).astype(np.uint8)


def binary(h, w, seed):
    """Every channel independently 0 or 255: bicubic's negative lobes overshoot both ends of clip8, the extrapolating blend clips,
    the IDCT's range limit saturates."""
    return (np.random.default_rng(seed).integers(0, 2, size=(h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)


def primaries(h, w, seed):
    """Saturated primaries and secondaries in 2x2 patches (luma far from every channel: the saturation blend extrapolates widely)."""
    pal = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [0, 0, 0], [255, 255, 255]], np.uint8)
    idx = np.random.default_rng(seed).integers(0, 8, size=((h + 1) // 2, (w + 1) // 2))
    return np.ascontiguousarray(pal[np.repeat(np.repeat(idx, 2, 0), 2, 1)[:h, :w]])


def content(kind, h, w, seed):
    return {'smooth': smooth, 'binary': binary, 'primaries': primaries}[kind](h, w, seed)


# ------------------------------------------------------------------------------------------------------------------
# A. JPEG back half.  A case is (name, stream bytes, dict(mode, w, h, ...)).
# ------------------------------------------------------------------------------------------------------------------
MODES = ('grey', '444', '422', '420')
_SUB = {'444': 0, '422': 1, '420': 2}


def jpeg_stream(arr, mode, **kw):
    if mode == 'grey':
        return jpeg_bytes(np.ascontiguousarray(arr[:, :, 0]), **kw)
    return jpeg_bytes(arr, subsampling=_SUB[mode], **kw)


def front_half_refuses(mode, w):
    """The supported subset leaves out chroma planes of <= 2 samples per row (jdsample.c replicates instead of filtering)."""
    return mode in ('422', '420') and (w + 1) // 2 <= 2


@functools.lru_cache(maxsize=None)
def a1_cases(mode):
    """Every (w, h) in 1..40 x 1..40: every residue of w and h mod 16 at least twice, chroma planes of 3..20 samples, every partial
    store group, block rows / columns of 1..8 real samples."""
    out = []
    for h in range(1, 41):
        for w in range(1, 41):
            q = (90, 50, 20)[(w + h) % 3]
            out.append(('a1-%s-%dx%d-q%d' % (mode, w, h, q), jpeg_stream(synth(w, h, 41 * w + h), mode, quality=q), dict(mode=mode, w=w, h=h)))
    return out


# (mode, w, h, nblocks, block0, edge): where a 256-block workgroup boundary falls.  'full': nblocks is a multiple of 256; 'tail': it is
# not; 'on': every component starts on a boundary; 'inside<c>': the first boundary lies strictly inside component c.
_A2 = [('grey', 128, 128, 256, (0, 0, 0), 'full'), ('grey', 136, 128, 272, (0, 0, 0), 'tail'), ('grey', 2040, 8, 255, (0, 0, 0), 'tail'),
       ('grey', 2049, 8, 257, (0, 0, 0), 'tail'), ('444', 128, 128, 768, (0, 256, 512), 'on'), ('420', 128, 128, 384, (0, 256, 320), 'on1'),
       ('420', 136, 120, 432, (0, 288, 360), 'inside0'), ('422', 200, 72, 468, (0, 234, 351), 'inside1'), ('444', 88, 64, 264, (0, 88, 176), 'inside2')]


def a2_edge_holds(info, edge):
    nb, b0 = int(info.nblocks), [int(v) for v in info.block0]
    if edge == 'full':
        return nb % 256 == 0
    if edge == 'tail':
        return nb % 256 != 0
    if edge == 'on':
        return b0[1] % 256 == 0 and b0[2] % 256 == 0 and b0[1] > 0 and b0[2] > b0[1]
    if edge == 'on1':
        return b0[1] == 256 and b0[2] % 256 != 0
    c = int(edge[-1])
    end = b0[c + 1] if c < 2 else nb
    return b0[c] < 256 < end and (c == 0 or b0[c] % 256 != 0)


@functools.lru_cache(maxsize=None)
def a2_cases():
    out = []
    for k, (mode, w, h, nb, b0, edge) in enumerate(_A2):
        out.append(('a2-%s-%dx%d' % (mode, w, h), jpeg_stream(synth(w, h, 7 + k), mode, quality=(85, 40)[k % 2]),
                    dict(mode=mode, w=w, h=h, nblocks=nb, block0=b0, edge=edge)))
    return out


def scale_dqt(data, factor):
    """The same stream with every (8-bit) quantisation table entry multiplied by `factor`: a decoder then dequantises to coefficients
    `factor` times larger than any encoder would have produced from 8-bit samples."""
    d = bytearray(data)
    i = 2
    while i + 4 <= len(d) and d[i] == 0xFF:
        marker, seglen = d[i + 1], (d[i + 2] << 8) | d[i + 3]
        if marker == 0xDB:
            j = i + 4
            while j < i + 2 + seglen:
                assert d[j] >> 4 == 0, '16-bit quantisation table'
                for t in range(j + 1, j + 65):
                    assert d[t] * factor <= 255
                    d[t] *= factor
                j += 65
        if marker == 0xDA:
            break
        i += 2 + seglen
    return bytes(d)


@functools.lru_cache(maxsize=None)
def a2x_cases():
    """Streams whose quantisation tables were scaled AFTER encoding (quality 100 writes all-1 tables): samples leave the IDCT more than
    384 beyond [0, 255], where jidctint.c's 10-bit range-limit table wraps (384..767 above the centre read 0) and libjpeg-turbo's
    SIMD inverse DCT -- what Pillow runs -- saturates.  Pillow decodes these streams like any other, so they carry the rule for
    out-of-range samples into the Pillow parity.  (Factors up to 6: the SIMD path also keeps dequantised coefficients and first-pass
    results in int16, which these streams respect.)"""
    out = []
    for mode, w, h, f in (('444', 40, 24, 6), ('grey', 33, 17, 5), ('420', 70, 50, 6), ('422', 70, 50, 4)):
        out.append(('a2x-%s-%dx%d-dqt*%d' % (mode, w, h, f), scale_dqt(jpeg_stream(binary(h, w, 3 * w + f), mode, quality=100), f),
                    dict(mode=mode, w=w, h=h)))
    return out


def a3_cases():
    """Output layouts: (name, stream, dict(mode, w, h, pitch, misalign))."""
    out = []
    for mode in MODES:
        for w in (1, 2, 3, 4, 5, 6, 7, 8, 9, 37, 40):
            if front_half_refuses(mode, w):
                continue
            data = jpeg_stream(synth(w, 5, 100 + w), mode, quality=80)
            for pitch in (3 * w, 3 * w + 1, (3 * w + 3) & ~3, 3 * w + 64):
                for mis in (0, 1, 2, 3):
                    out.append(('a3-%s-w%d-p%d-o%d' % (mode, w, pitch, mis), data, dict(mode=mode, w=w, h=5, pitch=pitch, misalign=mis)))
    return out


def a5_cases():
    return [('a5-1x1', jpeg_stream(synth(1, 1, 1), '444', quality=90), dict(mode='444', w=1, h=1)),
            ('a5-2049x8-grey', jpeg_stream(synth(2049, 8, 2), 'grey', quality=75), dict(mode='grey', w=2049, h=8)),
            ('a5-640x480-420', jpeg_stream(synth(640, 480, 3), '420', quality=85), dict(mode='420', w=640, h=480)),
            ('a5-17x23-422', jpeg_stream(synth(17, 23, 4), '422', quality=60), dict(mode='422', w=17, h=23)),
            ('a5-8x8', jpeg_stream(synth(8, 8, 5), '444', quality=95), dict(mode='444', w=8, h=8))]


# ---- A7: synthetic coefficients on the layout of real streams.  The encoder never produces large coefficients: ENCODER_MAX is a chosen
# bound just above the largest dequantised magnitude measured over A1 + A2 and over quality 1, 2, 5, 100 and all-1 / all-255 / mixed
# `qtables=` streams (1 025 with Pillow 12.2; tests/test_input_side_cpu.py re-measures and fails if a stream exceeds the bound); the
# synthetic arrays reach four times the bound.
ENCODER_MAX = 1026
A7_MAGNITUDE = 4 * ENCODER_MAX
A7_LAYOUTS = (('grey', 40, 24), ('422', 70, 50), ('420', 70, 50))


def a7_coefs(info, seed):
    """int16 coefficients whose DEQUANTISED values are seeded random within +-A7_MAGNITUDE (sparse towards high frequencies, as real
    blocks are), a few blocks holding a single extreme DC or a single extreme AC(7,7)."""
    g = np.random.default_rng(seed)
    nb = int(info.nblocks)
    out = np.zeros((nb, 64), np.int16)
    b0 = [int(v) for v in info.block0] + [nb]
    ncomp = int(info.ncomp)
    for c in range(ncomp):
        qt = np.array(info.qt[c][:], dtype=np.int64)
        lim = A7_MAGNITUDE // qt                                   # |coef * qt| <= A7_MAGNITUDE
        lo, hi = b0[c], (b0[c + 1] if ncomp == 3 else nb)
        n = hi - lo
        v = (g.uniform(-1.0, 1.0, size=(n, 64)) * lim).astype(np.int64)
        v[g.random((n, 64)) < 0.5] = 0
        for k, b in enumerate(range(0, n, 5)):                     # every fifth block: one extreme coefficient alone
            v[b] = 0
            v[b, (0, 63)[k % 2]] = (lim[(0, 63)[k % 2]]) * (1, -1)[(k // 2) % 2]
        out[lo:hi] = v
    return out.reshape(-1)


def idct_intermediates_max(info, coefs):
    """Largest magnitude of any value the restated IDCT multiplies (operands of the kernel's 24-bit multiplies): dequantised coefficients,
    their pairwise sums, the first-pass results and their sums."""
    worst = 0
    ncomp = 3 if int(info.ncomp) == 3 else 1
    b0 = [int(v) for v in info.block0] + [int(info.nblocks)]
    for c in range(ncomp):
        qt = np.array(info.qt[c][:], dtype=np.int64).reshape(1, 8, 8)
        lo, hi = b0[c], (b0[c + 1] if ncomp == 3 else int(info.nblocks))
        x = coefs[lo * 64:hi * 64].astype(np.int64).reshape(-1, 8, 8) * qt
        worst = max(worst, _operand_max([x[:, r, :] for r in range(8)]))
        ws = np.stack(JB._idct_1d(*[x[:, r, :] for r in range(8)], JB.CONST_BITS - JB.PASS1_BITS), axis=1)
        worst = max(worst, _operand_max([ws[:, :, k] for k in range(8)]))
    return worst


def idct_fits_int32(info, coefs):
    """True when the restated IDCT evaluated in wrapping int32 arithmetic (what the kernel and libjpeg's 32-bit builds have) gives the
    same samples as in int64: no product or sum of the two passes leaves 32 bits."""
    ncomp = 3 if int(info.ncomp) == 3 else 1
    b0 = [int(v) for v in info.block0] + [int(info.nblocks)]
    for c in range(ncomp):
        qt = np.array(info.qt[c][:], dtype=np.int64).reshape(1, 8, 8)
        lo, hi = b0[c], (b0[c + 1] if ncomp == 3 else int(info.nblocks))
        x = coefs[lo * 64:hi * 64].astype(np.int64).reshape(-1, 8, 8) * qt
        res = []
        for dt in (np.int64, np.int32):
            with np.errstate(over='ignore'):
                xs = x.astype(dt)
                ws = np.stack(JB._idct_1d(*[xs[:, r, :] for r in range(8)], JB.CONST_BITS - JB.PASS1_BITS), axis=1)
                res.append(np.stack(JB._idct_1d(*[ws[:, :, k] for k in range(8)], JB.CONST_BITS + JB.PASS1_BITS + 3), axis=2).astype(np.int64))
        if not np.array_equal(res[0], res[1]):
            return False
    return True


def _operand_max(i):
    ops = [i[1], i[2], i[3], i[5], i[6], i[7], i[2] + i[6], i[7] + i[1], i[5] + i[3], i[7] + i[3], i[5] + i[1], i[7] + i[3] + i[5] + i[1]]
    return max(int(np.abs(o).max()) for o in ops)


# ------------------------------------------------------------------------------------------------------------------
# B. Test transform.  A case is (name, (h, w, kind, seed), dict(resize_short, crop)); `image_of(case)` builds the pixels.
# ------------------------------------------------------------------------------------------------------------------
B1_SETTINGS = ((16, 16), (16, 17), (16, 18), (24, 27), (32, 36))          # (crop, resize_short)
_B1_BIG = (63, 64, 65, 127, 128, 129, 200, 401)
_B1_SMALL = (1, 2, 16, 40)
_B1_DOWN = (128, 129, 200, 401)           # both axes large: down-scaling by >= 10 (kernel sizes past 41 taps) needs a long SHORT side


def _b1_sizes():
    s = [(h, w) for h in range(1, 41) for w in range(1, 41) if (7 * h + 3 * w) % 4 != 0]
    s += [(a, b) for a in _B1_BIG for b in _B1_SMALL] + [(b, a) for a in _B1_BIG for b in _B1_SMALL]
    s += [(a, b) for a in _B1_DOWN for b in _B1_DOWN]
    return s


def b1_cases(crop, resize_short):
    out = []
    for k, (h, w) in enumerate(_b1_sizes()):
        kind = ('binary', 'smooth')[k % 2]
        out.append(('b1-c%d-s%d-%dx%d-%s' % (crop, resize_short, h, w, kind), (h, w, kind, 1000 * h + w), dict(resize_short=resize_short, crop=crop)))
    return out


def b1_subset(crop, resize_short):
    """The cases the (slow) numpy restatement runs on: every fifth small pair and every large one whose resized image stays small;
    tests/test_input_side_cpu.py asserts the table conditions on this subset as well."""
    out = []
    for k, c in enumerate(b1_cases(crop, resize_short)):
        h, w = c[1][:2]
        nh, nw = IO.resized_size(h, w, resize_short)
        if max(nh, nw) > 700:
            continue
        if k % 5 == 0 or max(h, w) > 40:
            out.append(c)
    return out


B2_SIZES = ((480, 640), (640, 480), (1201, 385), (385, 1201), (384, 384), (385, 384), (426, 426), (17, 23), (1080, 1920))


def b2_cases(resize_short):
    return [('b2-s%d-%dx%d' % (resize_short, h, w), (h, w, ('smooth', 'binary')[k % 2], 77 * k + resize_short), dict(resize_short=resize_short, crop=384))
            for k, (h, w) in enumerate(B2_SIZES)]


def image_of(case):
    h, w, kind, seed = case[1]
    return content(kind, h, w, seed)


def first_tap(in_size, out_size, x0, support=2.0):
    """Resample.c precompute_coeffs: first source index of output position x0."""
    scale = in_size / out_size
    sup = support * max(scale, 1.0)
    return max(int((x0 + 0.5) * scale - sup + 0.5), 0)


def ksize_of(in_size, out_size, support=2.0):
    return int(math.ceil(support * max(in_size / out_size, 1.0))) * 2 + 1


def b1_conditions(cases):
    """What the B1 table must keep satisfying, per axis (0 = vertical, 1 = horizontal); returns a list of violated conditions."""
    seen = [dict(mod4=set(), dirs=set(), up=set(), down=False, first=False) for _ in range(2)]
    ks = set()
    for _, (h, w, _k, _s), pr in cases:
        nh, nw = IO.resized_size(h, w, pr['resize_short'])
        origin = IO.crop_origin(nh, nw, pr['crop'])
        for ax, (n_in, n_out) in enumerate(((h, nh), (w, nw))):
            d = n_out - pr['crop']
            assert d >= 0
            s = seen[ax]
            s['mod4'].add(d % 4)
            if d % 2:
                s['dirs'].add('down' if origin[ax] == d // 2 else 'up')
                assert origin[ax] in (d // 2, d // 2 + 1)
            if n_out > n_in and n_in in (1, 2):
                s['up'].add(n_in)
            s['down'] |= n_in >= 10 * n_out
            s['first'] |= first_tap(n_in, n_out, origin[ax]) > 0
            ks.add(ksize_of(n_in, n_out))
    bad = []
    for ax, s in enumerate(seen):
        if not {1, 3} <= s['mod4']:
            bad.append('axis %d: out - crop mod 4 only %s' % (ax, sorted(s['mod4'])))
        if s['dirs'] != {'down', 'up'}:
            bad.append('axis %d: py_round_half directions %s' % (ax, sorted(s['dirs'])))
        if s['up'] != {1, 2}:
            bad.append('axis %d: up-scaling from %s' % (ax, sorted(s['up'])))
        if not s['down']:
            bad.append('axis %d: no down-scaling by >= 10' % ax)
        if not s['first']:
            bad.append('axis %d: row_first > 0 never' % ax)
    if min(ks) != 5 or max(ks) < 41:
        bad.append('ksize range %d..%d' % (min(ks), max(ks)))
    return bad


def transform_restated(img, size, crop, M=IO):
    """The test transform from the numpy restatement (module M: oracle.image_oracle or a mutant of it)."""
    h, w = img.shape[:2]
    nh, nw = M.resized_size(h, w, size)
    top, left = M.crop_origin(nh, nw, crop)
    u8 = M.resample_restated(img, nh, nw)[top:top + crop, left:left + crop]
    return M._finish(u8)


# ------------------------------------------------------------------------------------------------------------------
# C. Train transform.  A case is (name, image array, dict(box, ops, flip, size)).
# ------------------------------------------------------------------------------------------------------------------
C_FACTORS = (0.0, 0.6, 0.9999, 1.0, 1.4, 2.5)


@functools.lru_cache(maxsize=None)
def c1_cases():
    out = []
    big = smooth(480, 320, 9)
    for size in (16, 24):
        for H, W, seed in ((40, 56, 1), (23, 17, 2)):
            img = smooth(H, W, seed)
            boxes = [('whole', (0, 0, H, W)), ('1x1', (H // 2, W // 3, 1, 1)), ('1xW', (H - 1, 0, 1, W)), ('Hx1', (0, W - 1, H, 1)),
                     ('last', (H - 7, W - 5, 7, 5)), ('corner1x1', (H - 1, W - 1, 1, 1))]
            if size <= min(H, W):
                boxes.append(('exact', (H - size, W - size, size, size)))
            for bname, box in boxes:
                for flip in (False, True):
                    out.append(('c1-s%d-%dx%d-%s-%s' % (size, H, W, bname, 'flip' if flip else 'noflip'), img, dict(box=box, ops=[], flip=flip, size=size)))
        box = (0, 0, 320, 320) if size == 16 else (0, 0, 480, 320)
        for flip in (False, True):
            out.append(('c1-s%d-480x320-down20-%s' % (size, 'flip' if flip else 'noflip'), big, dict(box=box, ops=[], flip=flip, size=size)))
    return out


@functools.lru_cache(maxsize=None)
def c2_cases():
    out = []
    g = np.random.default_rng(2)
    imgs = (('binary', binary(20, 20, 4)), ('primaries', primaries(20, 20, 5)))
    for cname, img in imgs:
        for order in itertools.permutations((0, 1, 2)):
            for t in range(36):
                fs = [C_FACTORS[int(i)] for i in g.integers(0, 6, 3)]
                ops = [(o, f) for o, f in zip(order, fs)]
                out.append(('c2-%s-%s-%d-%s' % (cname, ''.join(map(str, order)), t, '/'.join('%g' % f for f in fs)), img,
                            dict(box=(0, 0, 20, 20), ops=ops, flip=bool(t & 1), size=16)))
        for op in (0, 1, 2):
            for f in C_FACTORS:
                out.append(('c2-%s-only%d-%g' % (cname, op, f), img, dict(box=(0, 0, 20, 20), ops=[(op, f)], flip=False, size=16)))
    return out


def planted_mean(size, n_low, low=10):
    """Grey size x size image with n_low pixels of `low` and the rest low + 1, scattered by a seeded permutation."""
    v = np.full(size * size, low + 1, np.uint8)
    v[np.random.default_rng(size + n_low).permutation(size * size)[:n_low]] = low
    return np.ascontiguousarray(np.repeat(v.reshape(size, size, 1), 3, axis=2))


def c3_cases():
    """Contrast mean at an exact half (int(mean + 0.5) rounds up) and just below it; at 384 the sum crosses all 16 waves."""
    out = []
    for size, lows in ((16, (128, 129)), (384, (384 * 192, 384 * 192 + 1))):
        for n_low in lows:
            img = planted_mean(size, n_low)
            for f in (0.6, 1.4):
                out.append(('c3-s%d-low%d-f%g' % (size, n_low, f), img, dict(box=(0, 0, size, size), ops=[(1, f)], flip=False, size=size)))
    return out


# ------------------------------------------------------------------------------------------------------------------
# Mutants: a restatement with ONE rule changed, made by substituting text in the oracle module's own source (the substituted text
# must occur exactly once) and executing the result as a module of its own -- never a copy of the oracle.
# ------------------------------------------------------------------------------------------------------------------


def mutant(mod, *subs):
    src = inspect.getsource(mod)
    for old, new in subs:
        assert src.count(old) == 1, 'mutant: %r occurs %d times in %s' % (old, src.count(old), mod.__name__)
        src = src.replace(old, new)
    m = types.ModuleType(mod.__name__ + '_mutant')
    m.__file__ = mod.__file__
    exec(compile(src, mod.__file__, 'exec'), m.__dict__)
    return m


def _fused_passes(M):
    """resample_restated with both passes accumulated exactly (no rounding to uint8 between them), from M's own weight tables."""
    def dense(n_in, n_out, filt):
        return dense_weights(M, n_in, n_out, filt)

    two_pass = M.resample_restated

    def fused(img, out_h, out_w, filt='bicubic'):
        if out_w == img.shape[1] or out_h == img.shape[0]:           # a single pass: nothing to fuse
            return two_pass(img, out_h, out_w, filt)
        acc = np.einsum('yh,hwc,xw->yxc', dense(img.shape[0], out_h, filt), img.astype(np.int64), dense(img.shape[1], out_w, filt))
        return np.clip((acc + (1 << (2 * M.PRECISION_BITS - 1))) >> (2 * M.PRECISION_BITS), 0, 255).astype(np.uint8)
    return fused


def jpeg_mutants():
    return {
        'chroma right neighbour from the padded column': mutant(JB, (':info.samp_h[c], :info.samp_w[c]]', ':info.samp_h[c], :]')),
        'bottom context row from the padded row': mutant(JB, (':info.samp_h[c], :info.samp_w[c]]', ':, :info.samp_w[c]]')),
        'h2v2 constants 8 and 7 exchanged': mutant(JB, ('last + 8) >> 4', 'last + 7) >> 4'), ('nxt + 7) >> 4', 'nxt + 8) >> 4'),
                                                   ('cs[:, 0] * 4 + 8) >> 4', 'cs[:, 0] * 4 + 7) >> 4'), ('cs[:, -1] * 4 + 7) >> 4', 'cs[:, -1] * 4 + 8) >> 4')),
        'h2v1 constants 1 and 2 exchanged': mutant(JB, ('left + 1) >> 2', 'left + 2) >> 2'), ('right + 2) >> 2', 'right + 1) >> 2')),
        # Pillow (libjpeg-turbo's SIMD inverse DCT) saturates out-of-range samples; the rule that can be got wrong is jidctint.c's table
        'range limit with the 10-bit wrap of the C path': mutant(JB, ('out = np.clip(x + 128, 0, 255)',
                                                                      'out = np.where((x & 1023) < 128, (x & 1023) + 128, np.where((x & 1023) < 512, 255, '
                                                                      'np.where((x & 1023) < 896, 0, (x & 1023) - 896)))')),
        'Cb and Cr exchanged': mutant(JB, ('ycc_to_rgb(yp, ch[0], ch[1])', 'ycc_to_rgb(yp, ch[1], ch[0])')),
        'descale without its rounding term': mutant(JB, ('return (x + (1 << (n - 1))) >> n', 'return x >> n')),
    }


# A mutant no table can kill, with the reason; tests/test_input_side_cpu.py checks the reason instead (equal weight tables).
EQUIVALENT_RESIZE_MUTANTS = {
    'xmin without the + 0.5': 'the only tap it adds lies at or beyond the filter support, where both filters are exactly 0: the window '
                              'starts one sample earlier with a zero weight; `xmax without the + 0.5` is its live sibling (it drops a real tap)',
}


def dense_weights(M, n_in, n_out, filt='bicubic'):
    """M.coeffs_restated as a dense (n_out, n_in) matrix: what the passes compute, whatever the window bookkeeping."""
    _, bounds, kk = M.coeffs_restated(n_in, n_out, filt)
    K = np.zeros((n_out, n_in), np.int64)
    for i in range(n_out):
        lo, n = bounds[i]
        K[i, lo:lo + n] = kk[i, :n]
    return K


def resize_mutants():
    fused = mutant(IO)
    fused.resample_restated = _fused_passes(fused)
    return {
        'crop origin rounded half-up': mutant(IO, ('return int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0))',
                                                   'return int(math.floor((h - crop) / 2.0 + 0.5)), int(math.floor((w - crop) / 2.0 + 0.5))')),
        'xmin without the + 0.5': mutant(IO, ('xmin = max(int(center - support + 0.5), 0)', 'xmin = max(int(center - support), 0)')),
        'xmax without the + 0.5': mutant(IO, ('xmax = min(int(center + support + 0.5), in_size) - xmin', 'xmax = min(int(center + support), in_size) - xmin')),
        'no lower clamp in clip8': mutant(IO, ('np.clip(acc >> PRECISION_BITS, 0, 255)', 'np.minimum(acc >> PRECISION_BITS, 255)')),
        'passes fused without the uint8 rounding between them': fused,
        'vertical pass first': mutant(IO, ('tmp = _pass(img, out_w, 1, filt) if out_w != img.shape[1] else img',
                                           'tmp = _pass(img, out_h, 0, filt) if out_h != img.shape[0] else img'),
                                      ('return _pass(tmp, out_h, 0, filt) if out_h != img.shape[0] else tmp',
                                       'return _pass(tmp, out_w, 1, filt) if out_w != img.shape[1] else tmp')),
        'long side round() instead of int()': mutant(IO, ('return int(size * h / w), size', 'return int(round(size * h / w)), size'),
                                                     ('return size, int(size * w / h)', 'return size, int(round(size * w / h))')),
    }


# Mirroring the box's pixels before the resize gives the mirrored result exactly when the horizontal weight table equals itself mirrored
# in both directions (the vertical pass does not see columns, the colour operations work per pixel or on whole-image means);
# tests/test_input_side_cpu.py asserts that for every (box width, size) of the tables.
EQUIVALENT_TRAIN_MUTANTS = {
    'flip applied to the source box': 'the integer weight table of the horizontal pass is mirror-symmetric for every box width of the tables, so '
                                      'flipping before the resize is the same arithmetic as flipping after it',
}


def train_mutants():
    return {
        'blend with a fused multiply-add': mutant(IO, ('t = in1.astype(np.float32) + a * d.astype(np.float32)',
                                                       't = (in1.astype(np.float64) + np.float64(a) * d.astype(np.float64)).astype(np.float32)')),
        'contrast mean floored': mutant(IO, ('/ L.size + 0.5)', '/ L.size)')),
        'luma without 0x8000': mutant(IO, (' + 0x8000) >> 16', ') >> 16')),
        'no clip when extrapolating': mutant(IO, ('return np.where(t <= 0.0, 0, np.where(t >= 255.0, 255, t)).astype(np.uint8)',
                                                  'return t.astype(np.int64).astype(np.uint8)')),
        'operations in fixed order 0, 1, 2': mutant(IO, ('for op, f in ops:\n        u8 = enhance_restated', 'for op, f in sorted(ops):\n        u8 = enhance_restated')),
        'flip applied to the source box': mutant(IO, ("np.ascontiguousarray(img[i:i + h, j:j + w]), size, size, 'bilinear')",
                                                      "np.ascontiguousarray(img[i:i + h, j:j + w][:, ::-1] if flip else img[i:i + h, j:j + w]), size, size, 'bilinear')"),
                                                 ('    if flip:\n        u8 = u8[:, ::-1]', '    if False:\n        u8 = u8[:, ::-1]')),
        # its live sibling: the box's POSITION mirrored in the image, the result not flipped
        'flip applied to the position of the source box': mutant(
            IO, ("np.ascontiguousarray(img[i:i + h, j:j + w]), size, size, 'bilinear')",
                 "np.ascontiguousarray(img[i:i + h, (img.shape[1] - j - w if flip else j):(img.shape[1] - j if flip else j + w)]), size, size, 'bilinear')"),
            ('    if flip:\n        u8 = u8[:, ::-1]', '    if False:\n        u8 = u8[:, ::-1]')),
    }
