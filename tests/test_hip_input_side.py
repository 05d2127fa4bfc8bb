"""Input side on the MI355X, through the C ABI itself (vitcap_amd._lib): vitcap_jpeg_backhalf, vitcap_image_preproc and
vitcap_image_train_preproc against PILLOW -- its decoder, its Image.resize, its ImageEnhance -- bit for bit, on the case tables of
oracle/input_side_cases.py: every small image size (every residue of the 16-pixel MCU, every partial store group, chroma planes of 3..20
samples), 256-block workgroup boundaries against component boundaries, every output pitch / base alignment (dword and byte store paths),
crops whose origin is not 0 on either axis, up-scaling from 1 and 2 pixels, 50-tap down-scaling, the colour operations at and beyond
their clipping points, a contrast mean planted on the exact half.  tests/test_input_side_cpu.py shows, without a GPU, that each of
these tables tells a restatement with one rule changed apart from Pillow.

Conventions (as in test_hip_gemm_forms.py): every output and every workspace lies inside a larger allocation pre-filled with the byte
0x7B; ONE torch.equal of the whole allocation against its expected image (sentinel outside, reference inside) proves the pixels and
the untouched surroundings -- pitch gaps, the bytes in front of and behind each image, the bytes behind workspace_bytes.  Every
comparison is exact.  The host-side queries vitcap_jpeg_backhalf_workspace_bytes, vitcap_image_preproc_workspace_bytes and
vitcap_image_train_preproc_workspace_bytes size every workspace here to the byte."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import image_oracle as IO
from oracle import input_side_cases as T
from oracle import jpeg_backhalf as JB

pytestmark = pytest.mark.gpu

SENT = 0x7B


def _L():
    from vitcap_amd import _lib
    return _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Arena(object):
    """Regions inside ONE sentinel-filled device allocation: each starts `mis` bytes past a 256-byte boundary and has at least 256
    sentinel bytes in front of and behind it.  `want` is the expected image of the whole allocation."""

    def __init__(self):
        self.size, self.regions, self.buf = 256, [], None

    def add(self, n, mis=0, name=''):
        off = self.size + mis
        self.regions.append((off, n, name))
        self.size = ((off + n + 255) & ~255) + 256
        return off

    def alloc(self):
        self.buf = torch.full((self.size,), SENT, dtype=torch.uint8, device='cuda')
        assert self.buf.data_ptr() % 256 == 0
        self.want = np.full(self.size, SENT, np.uint8)
        return self

    def ptr(self, off):
        return self.buf.data_ptr() + off

    def rows(self, off, h, nbytes, pitch):
        """The expected image's h rows of nbytes at `off`, pitch apart, as a writable (h, nbytes) view."""
        return np.lib.stride_tricks.as_strided(self.want[off:], shape=(h, nbytes), strides=(pitch, 1))

    def check(self, what=''):
        if torch.equal(self.buf, torch.from_numpy(self.want).cuda()):
            return
        got = self.buf.cpu().numpy()
        bad = np.nonzero(got != self.want)[0]
        first = int(bad[0])
        where = 'guard bytes'
        for off, n, name in self.regions:
            if off - 256 <= first < off + n + 256:
                where = '%s at byte %d of its %d (negative / past the end: guard)' % (name, first - off, n)
                break
        raise AssertionError('%s: %d bytes differ, first at %d: %s, got %d want %d' % (what, bad.size, first, where, got[first], self.want[first]))

    def untouched_outside(self, off, n):
        """For a workspace: its own bytes are the kernels' to use, everything around them must still be the sentinel."""
        return bool((self.buf[:off] == SENT).all()) and bool((self.buf[off + n:] == SENT).all())


# ==================================================================================================================
# A. vitcap_jpeg_backhalf
# ==================================================================================================================
def _decode(cases):
    """[(name, stream, parameters)] -> [(name, info, coefs, Pillow's pixels)]; asserts the front half refuses exactly what lies outside
    the supported subset (subsampled chroma rows of <= 2 samples)."""
    from vitcap_amd import jpegdec as J
    out = []
    for name, data, pr in cases:
        got = J.decode_coefs(data)
        assert (got is None) == T.front_half_refuses(pr['mode'], pr['w']), name
        if got is not None:
            out.append((name, got[0], got[1], T.pillow_rgb(data)))
    return out


def _jpeg_descs(items, layouts=None):
    """Uploads the coefficients (16-byte aligned, one copy) and lays the outputs out in an Arena.  -> (desc array, arena, geometry, keep)."""
    L = _L()
    B = len(items)
    offs, tot = [], 0
    for _, info, co, _ in items:
        assert co.dtype == np.int16 and co.size == info.nblocks * 64
        offs.append(tot)
        tot += (co.nbytes + 15) & ~15
    host = np.zeros(tot, np.uint8)
    for o, (_, _, co, _) in zip(offs, items):
        host[o:o + co.nbytes] = co.view(np.uint8)
    dco = torch.from_numpy(host).cuda()
    assert dco.data_ptr() % 16 == 0
    arena, geo = Arena(), []
    for k, (name, info, _, _) in enumerate(items):
        w, h = int(info.width), int(info.height)
        pitch, mis = layouts[k] if layouts else ((3 * w + 3) & ~3, 0)
        geo.append((arena.add((h - 1) * pitch + 3 * w, mis, name), h, w, pitch))
    arena.alloc()
    desc = (L.JpegImage * B)()
    for k, (_, info, _, _) in enumerate(items):
        desc[k].info = info
        desc[k].coefs, desc[k].rgb, desc[k].pitch = dco.data_ptr() + offs[k], arena.ptr(geo[k][0]), geo[k][3]
    return desc, arena, geo, dco


class _BackhalfCall(object):
    """One vitcap_jpeg_backhalf call in three steps, so that several calls can be prepared first and then issued with nothing between
    them: the constructor does every allocation, upload and expected image (all torch work), `launch` is the C-ABI call alone,
    `finish` synchronises and checks pixels, guards and the bytes around the workspace of exactly the reported size."""

    def __init__(self, items, layouts=None, what='jpeg_backhalf'):
        L = _L()
        self.what, self.B = what, len(items)
        self.desc, self.arena, geo, self.keep = _jpeg_descs(items, layouts)
        self.need = L.lib.vitcap_jpeg_backhalf_workspace_bytes(self.desc, self.B)
        self.ws = Arena()
        self.wo = self.ws.add(self.need)
        self.ws.alloc()
        for (off, h, w, pitch), (_, _, _, want) in zip(geo, items):
            self.arena.rows(off, h, 3 * w, pitch)[:] = want.reshape(h, 3 * w)
        self.stream = _stream()

    def launch(self):
        L = _L()
        L.check(L.lib.vitcap_jpeg_backhalf(self.desc, self.B, C.c_void_p(self.ws.ptr(self.wo)), self.need, self.stream), self.what)

    def finish(self):
        torch.cuda.synchronize()
        self.arena.check(self.what)
        assert self.ws.untouched_outside(self.wo, self.need), '%s wrote outside its %d workspace bytes' % (self.what, self.need)


def _run_backhalf(items, layouts=None, what='jpeg_backhalf'):
    call = _BackhalfCall(items, layouts, what)
    call.launch()
    call.finish()


@pytest.mark.parametrize('mode', T.MODES)
def test_a1_every_small_size_equals_pillow(mode):
    items = _decode(T.a1_cases(mode))
    assert len(items) == (1600 if mode in ('grey', '444') else 1440)
    _run_backhalf(items, what='A1 ' + mode)


def test_a2_workgroup_boundaries_against_component_boundaries():
    cases = T.a2_cases()
    items = _decode(cases)
    for (name, info, _, _), (_, _, pr) in zip(items, cases):
        assert int(info.nblocks) == pr['nblocks'] and (info.ncomp == 1 or tuple(info.block0) == pr['block0']), name
        assert T.a2_edge_holds(info, pr['edge']), (name, pr['edge'])
    _run_backhalf(items, what='A2')


def test_a2x_out_of_range_samples_saturate_as_pillow_does():
    """Streams with inflated quantisation tables: samples leave the IDCT past the point where jidctint.c's 10-bit range-limit table wraps.
    Pillow (libjpeg-turbo's SIMD inverse DCT) saturates there, and so must the kernel."""
    items = _decode(T.a2x_cases())
    assert all((want == 0).any() and (want == 255).any() for _, _, _, want in items)
    _run_backhalf(items, what='A2x')


def test_a3_every_pitch_and_base_alignment():
    cases = T.a3_cases()
    items = _decode(cases)
    assert len(items) == len(cases) == 16 * (11 + 11 + 7 + 7)
    layouts = [(pr['pitch'], pr['misalign']) for _, _, pr in cases]
    assert {(p % 4 == 0, m == 0) for p, m in layouts} == {(True, True), (True, False), (False, True), (False, False)}
    _run_backhalf(items, layouts, what='A3')


def _batch_444_32():
    return _decode([('a4-%d' % k, T.jpeg_stream(T.synth(32, 32, 60 + k), '444', quality=(90, 30)[k % 2]), dict(mode='444', w=32, h=32)) for k in range(8)])


def test_a4_workspace_to_the_byte():
    """Planes of exactly 1 024 bytes: no alignment padding between them, the chroma fetch's over-read lands in a neighbour's samples.
    The exact size decodes (every _run_backhalf call uses it and checks the 256 bytes behind it); one byte less is refused."""
    L = _L()
    items = _batch_444_32()
    assert all(int(i.blocks_w[c]) * int(i.blocks_h[c]) * 64 == 1024 for _, i, _, _ in items for c in range(3))
    _run_backhalf(items, what='A4')
    desc, arena, _, keep = _jpeg_descs(items)
    need = L.lib.vitcap_jpeg_backhalf_workspace_bytes(desc, len(items))
    ws = Arena()
    wo = ws.add(need)
    ws.alloc()
    assert L.lib.vitcap_jpeg_backhalf(desc, len(items), C.c_void_p(ws.ptr(wo)), need - 1, _stream()) != 0
    assert b'workspace too small' in L.lib.vitcap_last_error()
    torch.cuda.synchronize()
    arena.check('A4 refused call')                        # nothing was written
    assert ws.untouched_outside(0, 0)


def test_a5_mixed_batch_in_both_orders_and_alone():
    items = _decode(T.a5_cases())
    _run_backhalf(items, what='A5 in order')
    _run_backhalf(items[::-1], what='A5 reversed')
    for it in items:
        _run_backhalf([it], what='A5 alone ' + it[0])


def test_a6_back_to_back_calls_share_the_plan_staging():
    """Two calls on one thread and stream with nothing between them -- buffers, uploads and expected images of BOTH are prepared first,
    no torch operation or synchronisation separates the two C-ABI calls: the second overwrites the pinned plan staging of the first,
    which it may do only after the event recorded behind the first call's plan upload.  Both results are checked afterwards."""
    first = _decode(T.a1_cases('420')[40 * 20 + 8:40 * 20 + 40] + T.a1_cases('444')[40 * 30:40 * 30 + 32])
    second = _decode(T.a5_cases()[2:5])
    assert len(first) == 64 and len(second) == 3
    c1, c2 = _BackhalfCall(first, what='A6 first (64 images)'), _BackhalfCall(second, what='A6 second (3 images)')
    torch.cuda.synchronize()                     # every upload and fill of both calls is done: from here on only the two C-ABI calls
    c1.launch()
    c2.launch()
    c1.finish()
    c2.finish()


def test_a7_synthetic_coefficients_four_times_the_encoder_maximum():
    """Coefficients no encoder writes (4x the largest dequantised magnitude measured, single extreme DC / AC(7,7) blocks) on the layouts of
    real streams, inside the kernel's stated 24-bit precondition (asserted on the CPU: test_a7_coefficient_bound_and_24_bit_precondition).
    Reference: the numpy restatement, which the CPU file pins against Pillow on all of A1 / A2 / A2x."""
    from vitcap_amd import jpegdec as J
    items = []
    for k, (mode, w, h) in enumerate(T.A7_LAYOUTS):
        info, _ = J.decode_coefs(T.jpeg_stream(T.synth(w, h, k), mode, quality=75))
        coefs = T.a7_coefs(info, 50 + k)
        assert T.idct_intermediates_max(info, coefs) < 1 << 23
        items.append(('a7-%s-%dx%d' % (mode, w, h), info, coefs, JB.backhalf(info, coefs)))
    _run_backhalf(items, what='A7')


def test_a8_refusals_leave_the_output_alone():
    L = _L()
    from vitcap_amd.jpegdec import JpegInfo
    base = _decode([('a8-444', T.jpeg_stream(T.synth(16, 16, 1), '444', quality=80), dict(mode='444', w=16, h=16)),
                    ('a8-422', T.jpeg_stream(T.synth(16, 16, 2), '422', quality=80), dict(mode='422', w=16, h=16))])

    def attempt(k, cause, edit=None, B=1, null_coefs=False, pitch=None):
        name, info, co, want = base[k]
        info = JpegInfo.from_buffer_copy(bytes(info))
        if edit:
            edit(info)
        desc, arena, _, keep = _jpeg_descs([(name, base[k][1], co, want)])
        desc[0].info = info
        if null_coefs:
            desc[0].coefs = None
        if pitch is not None:
            desc[0].pitch = pitch
        need = max(L.lib.vitcap_jpeg_backhalf_workspace_bytes(desc, 1), 4096)
        ws = Arena()
        wo = ws.add(need)
        ws.alloc()
        rc = L.lib.vitcap_jpeg_backhalf(desc, B, C.c_void_p(ws.ptr(wo)), need, _stream())
        msg = L.lib.vitcap_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and cause in msg, (cause, rc, msg)
        arena.check('A8 ' + cause)
        assert ws.untouched_outside(0, 0), 'A8 %s: the workspace was written' % cause

    def set_(field, value, idx=None):
        def f(info):
            if idx is None:
                setattr(info, field, value)
            else:
                getattr(info, field)[idx] = value
        return f

    attempt(0, 'inconsistent vitcap_jpeg_info', set_('abi', 99))
    attempt(0, 'inconsistent vitcap_jpeg_info', lambda i: setattr(i, 'nblocks', i.nblocks + 1))
    attempt(0, 'inconsistent vitcap_jpeg_info', lambda i: setattr(i, 'nblocks', i.nblocks - 1))

    def h1v2(info):
        info.hs[0], info.vs[0] = 1, 2
    attempt(0, 'inconsistent vitcap_jpeg_info', h1v2)

    def narrow_chroma(info):
        assert info.hs[0] == 2
        info.samp_w[1] = info.samp_w[2] = 2
    attempt(1, 'inconsistent vitcap_jpeg_info', narrow_chroma)
    attempt(0, 'bad descriptor', pitch=3 * 16 - 1)
    attempt(0, 'bad descriptor', null_coefs=True)
    attempt(0, 'bad arguments', B=0)


# ==================================================================================================================
# B. vitcap_image_preproc
# ==================================================================================================================
def _upload_images(imgs, layouts=None, seed=0):
    """uint8 (H,W,3) arrays into one device buffer, image k at pitch / base misalignment layouts[k] (default: contiguous, aligned), the
    bytes between rows and images random.  -> (Image descriptor array, device buffer)."""
    L = _L()
    B = len(imgs)
    offs, tot = [], 256
    for k, im in enumerate(imgs):
        h, w = im.shape[:2]
        pitch, mis = layouts[k] if layouts else (3 * w, 0)
        offs.append((tot + mis, pitch))
        tot = ((tot + mis + (h - 1) * pitch + 3 * w + 255) & ~255) + 256
    host = np.random.default_rng(seed).integers(0, 256, size=tot, dtype=np.uint8)
    for (o, pitch), im in zip(offs, imgs):
        h, w = im.shape[:2]
        np.lib.stride_tricks.as_strided(host[o:], shape=(h, 3 * w), strides=(pitch, 1))[:] = im.reshape(h, 3 * w)
    dev = torch.from_numpy(host).cuda()
    desc = (L.Image * B)()
    for k, ((o, pitch), im) in enumerate(zip(offs, imgs)):
        desc[k] = L.Image(dev.data_ptr() + o, im.shape[0], im.shape[1], pitch)
    return desc, dev


def _norm_bytes(f32, bf16):
    t = torch.from_numpy(np.ascontiguousarray(f32))
    if bf16:
        return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint8).reshape(-1)      # round-to-nearest-even of the fp32 result
    return t.numpy().view(np.uint8).reshape(-1)


def _outputs(B, size, bf16, with_u8):
    out = Arena()
    oo = out.add(B * 3 * size * size * (2 if bf16 else 4), name='out')
    ou = out.add(B * 3 * size * size, name='out_u8')
    out.alloc()
    return out, oo, ou


def _run_preproc(imgs, resize_short, crop, bf16=False, with_u8=True, layouts=None, what='image_preproc'):
    """One vitcap_image_preproc call (exact workspace, guarded outputs) against Pillow; returns the arena for further comparisons."""
    L = _L()
    B = len(imgs)
    desc, keep = _upload_images(imgs, layouts)
    out, oo, ou = _outputs(B, crop, bf16, with_u8)
    need = L.lib.vitcap_image_preproc_workspace_bytes(desc, B, resize_short, crop)
    ws = Arena()
    wo = ws.add(need)
    ws.alloc()
    L.check(L.lib.vitcap_image_preproc(desc, B, resize_short, crop, int(bf16), C.c_void_p(out.ptr(oo)), C.c_void_p(out.ptr(ou)) if with_u8 else None,
                                       C.c_void_p(ws.ptr(wo)), need, _stream()), what)
    refs = [IO.transform_reference(im, resize_short, crop) for im in imgs]
    out.want[oo:oo + B * 3 * crop * crop * (2 if bf16 else 4)] = _norm_bytes(np.stack([r[1] for r in refs]), bf16)
    if with_u8:
        out.want[ou:ou + B * 3 * crop * crop] = np.stack([r[0] for r in refs]).reshape(-1)
    torch.cuda.synchronize()
    out.check(what)
    assert ws.untouched_outside(wo, need), '%s wrote outside its %d workspace bytes' % (what, need)
    del keep
    return out


@pytest.mark.parametrize('crop,resize_short', T.B1_SETTINGS)
def test_b1_small_crops_equal_pillow(crop, resize_short):
    cases = T.b1_cases(crop, resize_short)
    assert 1200 <= len(cases) <= 2048 and T.b1_conditions(cases) == []
    _run_preproc([T.image_of(c) for c in cases], resize_short, crop, what='B1 crop %d resize_short %d' % (crop, resize_short))


@pytest.mark.parametrize('resize_short', [384, 426, 438])
def test_b2_model_size_equals_pillow(resize_short):
    _run_preproc([T.image_of(c) for c in T.b2_cases(resize_short)], resize_short, 384, what='B2 resize_short %d' % resize_short)


def _few_images():
    return [T.smooth(37, 53, 1), T.binary(64, 29, 2), T.smooth(200, 40, 3)]


def test_b3_source_pitch_and_odd_base():
    imgs = _few_images()
    a = _run_preproc(imgs, 27, 24, what='B3 contiguous')
    for extra in (1, 61):
        b = _run_preproc(imgs, 27, 24, layouts=[(3 * im.shape[1] + extra, 1 + 2 * k) for k, im in enumerate(imgs)], what='B3 pitch 3w + %d, odd base' % extra)
        assert torch.equal(a.buf, b.buf)


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('with_u8', [False, True], ids=['no_u8', 'u8'])
def test_b4_output_forms(bf16, with_u8):
    """fp32, bf16 (= round-to-nearest-even of the fp32 result), out_u8 null and given: the output that is not asked for stays the
    sentinel (the arena holds both regions either way), guards and the bytes behind the exact workspace too."""
    _run_preproc(_few_images() + [T.binary(17, 23, 5)], 18, 16, bf16=bf16, with_u8=with_u8, what='B4')


def test_b5_refusals_leave_the_outputs_alone():
    L = _L()
    imgs = _few_images()

    def attempt(cause, imgs=imgs, resize_short=27, crop=24, short=0, edit=None, null_out=False):
        B = len(imgs)
        desc, keep = _upload_images(imgs)
        if edit:
            edit(desc)
        out, oo, ou = _outputs(B, max(crop, 1), False, True)
        need = max(L.lib.vitcap_image_preproc_workspace_bytes(desc, B, resize_short, max(crop, 1)), 4096)
        ws = Arena()
        wo = ws.add(need)
        ws.alloc()
        rc = L.lib.vitcap_image_preproc(desc, B, resize_short, crop, 0, C.c_void_p(out.ptr(oo)), C.c_void_p(out.ptr(ou)), C.c_void_p(ws.ptr(wo)),
                                        L.lib.vitcap_image_preproc_workspace_bytes(desc, B, resize_short, max(crop, 1)) - short if short else need, _stream())
        msg = L.lib.vitcap_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and cause in msg, (cause, rc, msg)
        out.check('B5 ' + cause)
        assert ws.untouched_outside(0, 0), 'B5 %s: the workspace was written' % cause

    attempt('workspace too small', short=1)
    attempt('smaller than the crop', imgs=[T.smooth(40, 400, 1)], resize_short=16, crop=24)

    def narrow(desc):
        desc[1].pitch = 3 * desc[1].width - 1
    attempt('bad descriptor', edit=narrow)

    def null_rgb(desc):
        desc[2].rgb = None
    attempt('bad descriptor', edit=null_rgb)
    attempt('bad arguments', crop=0)


# ==================================================================================================================
# C. vitcap_image_train_preproc
# ==================================================================================================================
def _augs(params):
    L = _L()
    aug = (L.TrainAug * len(params))()
    for a, pr in zip(aug, params):
        a.top, a.left, a.height, a.width = [int(v) for v in pr['box']]
        a.flip = int(bool(pr['flip']))
        ops = list(pr['ops'])
        for o in range(3):
            a.op[o], a.factor[o] = (int(ops[o][0]), float(ops[o][1])) if o < len(ops) else (-1, 1.0)
    return aug


def _run_train(cases, size, bf16=False, with_u8=True, what='image_train_preproc'):
    L = _L()
    B = len(cases)
    assert all(pr['size'] == size for _, _, pr in cases)
    uniq = {}
    for _, img, _ in cases:                                   # many cases share an image: upload each once
        uniq.setdefault(id(img), (len(uniq), img))
    udesc, keep = _upload_images([im for _, im in uniq.values()])
    desc = (L.Image * B)()
    for k, (_, img, _) in enumerate(cases):
        desc[k] = udesc[uniq[id(img)][0]]
    aug = _augs([pr for _, _, pr in cases])
    out, oo, ou = _outputs(B, size, bf16, with_u8)
    need = L.lib.vitcap_image_train_preproc_workspace_bytes(desc, aug, B, size)
    ws = Arena()
    wo = ws.add(need)
    ws.alloc()
    L.check(L.lib.vitcap_image_train_preproc(desc, aug, B, size, int(bf16), C.c_void_p(out.ptr(oo)), C.c_void_p(out.ptr(ou)) if with_u8 else None,
                                             C.c_void_p(ws.ptr(wo)), need, _stream()), what)
    refs = [IO.train_transform_reference(img, pr['box'], pr['ops'], pr['flip'], size) for _, img, pr in cases]
    out.want[oo:oo + B * 3 * size * size * (2 if bf16 else 4)] = _norm_bytes(np.stack([r[1] for r in refs]), bf16)
    if with_u8:
        out.want[ou:ou + B * 3 * size * size] = np.stack([r[0] for r in refs]).reshape(-1)
    torch.cuda.synchronize()
    try:
        out.check(what)
    except AssertionError as e:
        got = out.buf[ou:ou + B * 3 * size * size].cpu().numpy().reshape(B, -1)
        bad = [cases[k][0] for k in range(B) if with_u8 and not np.array_equal(got[k], refs[k][0].reshape(-1))]
        raise AssertionError('%s; cases whose bytes differ: %s' % (e, bad[:8]))
    assert ws.untouched_outside(wo, need), '%s wrote outside its %d workspace bytes' % (what, need)
    del keep


@pytest.mark.parametrize('size', [16, 24])
def test_c1_boxes_equal_pillow(size):
    cases = [c for c in T.c1_cases() if c[2]['size'] == size]
    assert len(cases) >= 26
    _run_train(cases, size, what='C1 size %d' % size)


def test_c2_colour_operations_equal_pillow():
    cases = T.c2_cases()
    assert len(cases) == 2 * (6 * 36 + 18) and {tuple(o for o, _ in pr['ops']) for _, _, pr in cases if len(pr['ops']) == 3} == {
        (0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)}
    _run_train(cases, 16, what='C2')


@pytest.mark.parametrize('size', [16, 384])
def test_c3_contrast_mean_planted_on_the_half(size):
    cases = [c for c in T.c3_cases() if c[2]['size'] == size]
    assert len(cases) == 4
    _run_train(cases, size, what='C3 size %d' % size)


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('with_u8', [False, True], ids=['no_u8', 'u8'])
def test_c4_output_forms(bf16, with_u8):
    _run_train(T.c1_cases()[:6] + T.c2_cases()[:10], 16, bf16=bf16, with_u8=with_u8, what='C4')


def test_c4_refusals_leave_the_outputs_alone():
    L = _L()
    img = T.smooth(40, 56, 1)
    good = dict(box=(0, 0, 40, 56), ops=[(0, 1.2), (1, 0.8)], flip=False)

    def attempt(cause, short=0, **change):
        pr = dict(good, **change)
        desc, keep = _upload_images([img])
        aug = _augs([pr])
        if 'raw_ops' in change:
            for o, (op, f) in enumerate(change['raw_ops']):
                aug[0].op[o], aug[0].factor[o] = op, f
        out, oo, ou = _outputs(1, 16, False, True)
        exact = L.lib.vitcap_image_train_preproc_workspace_bytes(desc, aug, 1, 16)
        need = max(exact, 4096)
        ws = Arena()
        wo = ws.add(need)
        ws.alloc()
        rc = L.lib.vitcap_image_train_preproc(desc, aug, 1, 16, 0, C.c_void_p(out.ptr(oo)), C.c_void_p(out.ptr(ou)), C.c_void_p(ws.ptr(wo)),
                                              exact - short if short else need, _stream())
        msg = L.lib.vitcap_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and cause in msg, (cause, rc, msg)
        out.check('C4 ' + cause)
        assert ws.untouched_outside(0, 0), 'C4 %s: the workspace was written' % cause

    attempt('workspace too small', short=1)
    attempt('lies outside', box=(1, 0, 40, 56))
    attempt('lies outside', box=(0, 50, 10, 7))
    attempt('lies outside', box=(0, 0, 0, 5))
    attempt('twice', ops=[(2, 1.0), (2, 1.1)])
    attempt('is not 0/1/2', raw_ops=[(3, 1.0)])
    attempt('negative enhancement factor', raw_ops=[(1, -0.25)])
