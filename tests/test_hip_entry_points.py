"""Direct parity tests of the C-ABI entry points that only whole-caption / whole-training-step runs used to reach
(docs/LAB_tests_entry_points.md): decode attention with tag keys, with several groups per image and away from S_vis = 578, the
K/V cache re-ordering, the CLS-rows form of the dense attention, the engine's data movers and the training step's small ops.

Every reference is computed on the CPU in fp32 / fp64 from the same bf16-rounded inputs; a second HIP kernel is only ever an
additional comparison.  Buffers that an entry point writes in part are pre-filled with a sentinel bit pattern (bf16 0x7B7B,
fp32 0x7B7B7B7B: finite, ~1e36, nothing here computes it) and everything outside the documented region must keep it.
Each toleranced comparison prints its largest error next to the bound (`pytest -s`), which is where the LAB note's figures are from.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT16 = 0x7B7B
SENT32 = 0x7B7B7B7B


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vitcap_amd import ops as o
    return o


@pytest.fixture(scope='module')
def lib(ops):
    from vitcap_amd._lib import lib as l
    return l


def _bf(t):
    return t.to(torch.bfloat16)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _report(what, err, tol):
    """Largest error and the bound at that element (tol may be a tensor: per-element bounds)."""
    err = err.double().flatten()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(err) if not torch.is_tensor(tol) else tol.double().flatten()
    i = int(err.argmax())
    ratio = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print('MEASURED %s: max err %.3e (bound there %.3e), largest err/bound %.3g' % (what, float(err[i]), float(tol[i]), ratio))


def _close(got, want, rtol, atol, what=''):
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    _report(what, err, tol)
    bad = ~(err <= tol)              # a NaN (or a left-over sentinel) is bad
    assert not bad.any(), '%s: %d/%d elements off, max err %.3e (want max %.3e), first bad idx %s' % (
        what, int(bad.sum()), bad.numel(), float(err.max()), float(want.abs().max()), bad.nonzero()[:4].tolist())


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    """Integer view for bit-for-bit comparisons (-0 != +0, NaN == NaN)."""
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _sent_bf16(*shape):
    return torch.full(shape, SENT16, dtype=torch.int16, device='cuda').view(torch.bfloat16)


def _sent_f32(*shape):
    return torch.full(shape, SENT32, dtype=torch.int32, device='cuda').view(torch.float32)


def _is_sent(t):
    b = _bits(t)
    return b == (SENT16 if b.dtype == torch.int16 else SENT32)


def _refused(lib, rc, needle):
    """A VC_REQUIRE said no: non-zero return, and vitcap_last_error() speaks of this entry point."""
    assert rc != 0
    msg = lib.vitcap_last_error()
    assert msg and needle in msg, msg


# ------------------------------------------------------------------------------------------------ a. decode attention with tag keys
def _decode_reference(vis, tag, cache, step, t, img):
    """fp32 reference of one decode step with the device's rounding points, as test_hip_ops.test_attn_decode_step builds it:
    keys = visual rows of the sequence's image | tag rows of the image | cached text 0..t-2 | this step's row 0 | [MASK] row."""
    from oracle import vitcap_oracle as O
    B = step.shape[0]
    parts_k = [vis[img][..., 768:1536].float()]
    parts_v = [vis[img][..., 1536:].float()]
    if tag is not None:
        parts_k.append(tag[img][..., 768:1536].float())
        parts_v.append(tag[img][..., 1536:].float())
    parts_k += [cache[:, :t - 1, 0].float(), step[:, :, 768:1536].float()]
    parts_v += [cache[:, :t - 1, 1].float(), step[:, :, 1536:].float()]
    K, V = torch.cat(parts_k, 1), torch.cat(parts_v, 1)
    q = step[..., :768].float().view(B, 2, 12, 64).transpose(1, 2)
    s = q @ K.view(B, -1, 12, 64).transpose(1, 2).transpose(-1, -2)
    s[:, :, 0, -1] = float('-inf')                        # row 0 (position t-1) does not see the [MASK] row
    return O.softmax_pv_rounded(s, V.view(B, -1, 12, 64).transpose(1, 2), O._R(True)).transpose(1, 2).reshape(B, 2, 768)


def _assert_cache_step(cache_dev, cache, step, t):
    """row t-1 now holds this step's real-token K/V, every other row is what it was"""
    c = cache_dev.cpu()
    assert torch.equal(_bits(c[:, t - 1, 0]), _bits(step[:, 0, 768:1536]))
    assert torch.equal(_bits(c[:, t - 1, 1]), _bits(step[:, 0, 1536:]))
    keep = [i for i in range(cache.shape[1]) if i != t - 1]
    assert torch.equal(_bits(c[:, keep]), _bits(cache[:, keep]))


# (B, seq_per_image, S_vis, n_tag, t, max_len, tag_len[0])
TAG_CASES = [
    (4, 2, 578, 50, 19, 20, 50),      # 50 + 20 <= 19 + 51: branch A; tag rows per IMAGE with two sequences per image
    (4, 2, 578, 7, 5, 20, 5 + 31),    # last tag_len[0] that still takes branch A at t = 5 ...
    (4, 2, 578, 7, 5, 20, 5 + 32),    # ... and the first that takes branch B
    (2, 1, 578, 1, 1, 20, 1),         # one tag key, first step
    (2, 1, 100, 7, 20, 41, 7),        # nkeys = 128: exactly one full sweep of 4 x 32 keys
    (2, 1, 100, 7, 21, 41, 7),        # nkeys = 129: one key into the second sweep
    (2, 1, 5, 0, 1, 20, None),        # nkeys = 7: every u > 0 slot of the sweep is clamped; no tag pointers at all
    (1, 1, 613, 50, 40, 41, 50),      # nkeys = 704 = MAXKEYS exactly
]


def _tag_inputs(B, spi, S, n_tag, t, L, tag_len0):
    n_img = B // spi
    vis = _bf(_rand((n_img, S, 2304), 130, 2.0))
    step = _bf(_rand((B, 2, 2304), 131 + t, 2.0))
    cache = _bf(_rand((B, L, 2, 768), 132, 2.0))
    tag_a = tag_b = tag_len = None
    if n_tag > 0:
        tag_a = _bf(_rand((n_img, n_tag, 2304), 133, 2.0))           # different seeds: the wrong branch misses by far
        tag_b = _bf(_rand((n_img, n_tag, 2304), 134, 2.0))
        use_a = tag_len0 + 20 <= t + 51
        # element 0 alone decides; the other images' lengths would pick the other branch
        tag_len = torch.full((n_img,), 0 if not use_a else 1000, dtype=torch.int64)
        tag_len[0] = tag_len0
    return vis, step, cache, tag_a, tag_b, tag_len


def _call_step_tags(lib, vis, step, cache_dev, out, B, S, t, L, spi, tag_a, tag_b, n_tag, tag_len):
    keep = [x.cuda().contiguous() if x is not None else None for x in (step.reshape(B * 2, 2304), vis.reshape(-1, 2304), tag_a, tag_b, tag_len)]
    rc = lib.vitcap_attn_decode_step_tags(_p(keep[0]), _p(keep[1]), _p(cache_dev), _p(out), B, S, t, L, spi, 0.125, _p(keep[2]),
                                          _p(keep[3]), n_tag, _p(keep[4]), _s())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('B,spi,S,n_tag,t,L,tag_len0', TAG_CASES, ids=lambda v: str(v))
def test_attn_decode_step_tags(lib, B, spi, S, n_tag, t, L, tag_len0):
    """vitcap_attn_decode_step_tags against the fp32 reference with the tag rows' K/V between the visual and the text keys:
    tag rows indexed by image (not by sequence), branch A iff tag_len[0] + 20 <= t + 51 with both sides of that boundary, and the
    sweep edges of the per-sequence kernel (7, 128, 129 and MAXKEYS = 704 keys).  2^-7 relative, 2e-3 absolute: the tolerance of
    test_attn_decode_step (fp32 summation order + one bf16 rounding of the output)."""
    vis, step, cache, tag_a, tag_b, tag_len = _tag_inputs(B, spi, S, n_tag, t, L, tag_len0)
    assert S + n_tag + t + 1 <= 704
    cache_dev = cache.cuda().contiguous()
    out = _sent_bf16(B * 2, 768)
    assert _call_step_tags(lib, vis, step, cache_dev, out, B, S, t, L, spi, tag_a, tag_b, n_tag, tag_len) == 0, lib.vitcap_last_error()
    img = torch.arange(B) // spi
    tag = None
    if n_tag > 0:
        tag = tag_a if tag_len0 + 20 <= t + 51 else tag_b
    want = _decode_reference(vis, tag, cache, step, t, img)
    _close(out.view(B, 2, 768), want, 2 ** -7, 2e-3, 'attn_decode_step_tags %s' % ((B, spi, S, n_tag, t, L, tag_len0),))
    _assert_cache_step(cache_dev, cache, step, t)


def test_attn_decode_step_tags_rejects(lib):
    """One key more than the score buffer holds (S_vis = 614 with 50 tags at t = 40: 705 keys) and one tag more than the 50 slots."""
    B, spi, S, n_tag, t, L, tl = TAG_CASES[-1]
    vis, step, cache, tag_a, tag_b, tag_len = _tag_inputs(B, spi, S + 1, n_tag + 1, t, L, tl)      # buffers cover either refused shape
    cache_dev = cache.cuda().contiguous()
    out = _sent_bf16(B * 2, 768)
    _refused(lib, _call_step_tags(lib, vis, step, cache_dev, out, B, 614, t, L, spi, tag_a, tag_b, 50, tag_len), b'attn_decode')
    _refused(lib, _call_step_tags(lib, vis, step, cache_dev, out, B, 100, t, L, spi, tag_a, tag_b, 51, tag_len), b'attn_decode')
    assert bool(_is_sent(out).all()) and torch.equal(_bits(cache_dev), _bits(cache))              # nothing ran


# ------------------------------------------------------------------------------------------------ b. beam groups, S_vis edges
# (n_images, seq_per_group, groups_per_image, S_vis, t, max_len)
GROUP_CASES = [
    (2, 3, 2, 578, 7, 20),     # small instantiation, two groups per image
    (2, 8, 3, 578, 19, 20),    # large instantiation (8 x 20 text pairs > 128), three groups per image
    (2, 5, 1, 17, 4, 20),      # two 16-key blocks: waves 2 and 3 own none; 15 clamped keys in the last block
    (2, 5, 1, 592, 4, 20),     # S_vis % 16 == 0: no clamped key in the last block
    (2, 5, 2, 608, 38, 40),    # S_vis = the padded width: no zero padding in vis_vt; large instantiation (max_len 40)
]


@pytest.mark.parametrize('n_img,spg,gpi,S,t,L', GROUP_CASES, ids=lambda v: str(v))
def test_attn_decode_beam_groups(ops, lib, n_img, spg, gpi, S, t, L):
    """vitcap_attn_decode_beam_groups (and vitcap_attn_beam_vt for that S_vis) against the fp32 reference with image index
    b // (seq_per_group * groups_per_image), and against the per-sequence kernel at seq_per_image = seq_per_group *
    groups_per_image on a copy of the cache: caches bit-equal, outputs within one bf16 ulp -- 2^-7 relative, 2e-3 absolute, as
    test_attn_decode_beams_vs_single_sequences states that bound (same softmax and bf16 rounding of P, another fp32 summation order)."""
    spi = spg * gpi
    B = n_img * spi
    vis = _bf(_rand((n_img, S, 2304), 140 + spg, 2.0))
    step = _bf(_rand((B, 2, 2304), 141 + t, 2.0))
    cache = _bf(_rand((B, L, 2, 768), 142, 2.0))
    c1, c2 = cache.cuda().contiguous(), cache.cuda().contiguous()
    step_d = step.reshape(B * 2, 2304).cuda().contiguous()
    vis_d = vis.reshape(n_img * S, 2304).cuda().contiguous()
    vt = _sent_bf16(n_img, 12, 64, 608)
    assert lib.vitcap_attn_beam_vt(_p(vis_d), _p(vt), n_img, S, _s()) == 0, lib.vitcap_last_error()
    # V^T per (image, head): [64 dims][608 keys], the keys behind S_vis zero
    want_vt = torch.zeros(n_img, 12, 64, 608, dtype=torch.bfloat16)
    want_vt[..., :S] = vis[..., 1536:].view(n_img, S, 12, 64).permute(0, 2, 3, 1)
    assert torch.equal(_bits(vt), _bits(want_vt)), 'vis_vt differs from the CPU transpose (S_vis = %d)' % S
    out = _sent_bf16(B * 2, 768)
    assert lib.vitcap_attn_decode_beam_groups(_p(step_d), _p(vis_d), _p(vt), _p(c1), _p(out), n_img, spg, gpi, S, t, L, 0.125, _s()) == 0, \
        lib.vitcap_last_error()
    torch.cuda.synchronize()
    img = torch.arange(B) // (spg * gpi)
    ref = _decode_reference(vis, None, cache, step, t, img)
    what = 'attn_decode_beam_groups %s' % ((n_img, spg, gpi, S, t, L),)
    _close(out.view(B, 2, 768), ref, 2 ** -7, 2e-3, what + ' vs fp32 reference')
    _assert_cache_step(c1, cache, step, t)
    single = ops.attn_decode_step(step_d, vis_d, c2, B, S, t, max_len=L, seq_per_image=spi)
    torch.cuda.synchronize()
    assert torch.equal(_bits(c1), _bits(c2))
    _close(out, single, 2 ** -7, 2e-3, what + ' vs per-sequence kernel')


@pytest.mark.parametrize('S', [16, 609])
def test_attn_decode_beam_groups_rejects(lib, S):
    n_img, spg, gpi, t, L = 1, 2, 1, 3, 20
    B = n_img * spg * gpi
    vis = torch.zeros(n_img * 609, 2304, dtype=torch.bfloat16, device='cuda')
    step = torch.zeros(B * 2, 2304, dtype=torch.bfloat16, device='cuda')
    cache = _sent_bf16(B, L, 2, 768)
    vt = torch.zeros(n_img, 12, 64, 608, dtype=torch.bfloat16, device='cuda')
    out = _sent_bf16(B * 2, 768)
    _refused(lib, lib.vitcap_attn_decode_beam_groups(_p(step), _p(vis), _p(vt), _p(cache), _p(out), n_img, spg, gpi, S, t, L, 0.125, _s()),
             b'attn_decode_beams')
    if S > 608:
        _refused(lib, lib.vitcap_attn_beam_vt(_p(vis), _p(vt), n_img, S, _s()), b'attn_beam_vt')
    torch.cuda.synchronize()
    assert bool(_is_sent(out).all()) and bool(_is_sent(cache).all())


# ------------------------------------------------------------------------------------------------ c. beam_reorder_cache
@pytest.mark.parametrize('t', [1, 7, 20])
def test_beam_reorder_cache(lib, t):
    """dst[l][s][:t] = src[l][parent[s]][:t] bit for bit; positions >= t of dst and all of src untouched."""
    layers, NS, L = 3, 10, 20
    src = _bf(_rand((layers, NS, L, 2, 768), 150, 2.0))
    parent = torch.tensor([3, 3, 0, 9, 1, 1, 1, 7, 2, 0], dtype=torch.int32)
    src_d, parent_d, dst = src.cuda().contiguous(), parent.cuda(), _sent_bf16(layers, NS, L, 2, 768)
    assert lib.vitcap_beam_reorder_cache(_p(src_d), _p(dst), _p(parent_d), layers, NS, L, t, _s()) == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(dst[:, :, :t]), _bits(src[:, parent.long(), :t]))
    assert bool(_is_sent(dst[:, :, t:]).all())
    assert torch.equal(_bits(src_d), _bits(src))


# ------------------------------------------------------------------------------------------------ d. attn_dense_fwd_rows
@functools.lru_cache(maxsize=None)
def _dense_case(B, S):
    """inputs, the whole-sequence kernel's output and the CPU emulation, once per (B, S)"""
    from oracle import vitcap_oracle as O
    from vitcap_amd import ops as o
    qkv = _bf(_rand((B, S, 2304), 160 + S, 2.0))
    qkv_d = qkv.reshape(B * S, 2304).cuda().contiguous()
    full = o.attn_dense(qkv_d, B, S)
    torch.cuda.synchronize()
    return qkv_d, full.cpu().view(B, S, 768), O.attn_rounded(qkv.float(), S, O._R(True))


@pytest.mark.parametrize('B,S,q_rows', [(2, 577, 1), (2, 577, 128), (2, 577, 129), (1, 577, 577), (2, 130, 1)])
def test_attn_dense_fwd_rows(lib, B, S, q_rows):
    """vitcap_attn_dense_fwd_rows (the last tag block: only the CLS row is read): the rows < q_rows equal vitcap_attn_dense_fwd's
    bit for bit and the CPU emulation within test_attn_dense's tolerance; rows behind the 128-row blocks covering q_rows are not written."""
    qkv_d, full, want = _dense_case(B, S)
    out = _sent_bf16(B * S, 768)
    assert lib.vitcap_attn_dense_fwd_rows(_p(qkv_d), _p(out), B, S, q_rows, 0.125, _s()) == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    out = out.cpu().view(B, S, 768)
    assert torch.equal(_bits(out[:, :q_rows]), _bits(full[:, :q_rows]))
    _close(out[:, :q_rows], want[:, :q_rows], 2 ** -7, 2e-3, 'attn_dense_fwd_rows %s vs emulation' % ((B, S, q_rows),))
    written = min(S, (q_rows + 127) // 128 * 128)
    assert bool(_is_sent(out[:, written:]).all())


# ------------------------------------------------------------------------------------------------ e. data movers (exact)
@pytest.mark.parametrize('geom', [dict(B=3, rows=578, cols=2304, src_img_rows=600, src_row0=3, ld_src=2304, src_col0=0,
                                       dst_img_rows=590, dst_row0=5, ld_dst=2312, dst_col0=8),
                                  dict(B=2, rows=5, cols=64, src_img_rows=7, src_row0=1, ld_src=768, src_col0=128,
                                       dst_img_rows=6, dst_row0=0, ld_dst=128, dst_col0=64)],
                         ids=['grid_stride_twice', 'column_sub_block'])
def test_copy_row_blocks(lib, geom):
    """bf16 row blocks between per-image layouts.  The first geometry has 578 * 288 = 166464 16-byte chunks per image, more than
    the 512-block grid covers at once (131072): the grid-stride loop runs twice."""
    g = geom
    src = _bf(_rand((g['B'] * g['src_img_rows'], g['ld_src']), 170))
    src_d = src.cuda()
    dst = _sent_bf16(g['B'] * g['dst_img_rows'], g['ld_dst'])
    args = lambda cols: (_p(src_d), g['src_img_rows'], g['src_row0'], g['ld_src'], g['src_col0'], _p(dst), g['dst_img_rows'],
                         g['dst_row0'], g['ld_dst'], g['dst_col0'], g['rows'], cols, g['B'], _s())
    _refused(lib, lib.vitcap_copy_row_blocks(*args(12)), b'copy_row_blocks')           # not whole 16-byte chunks
    torch.cuda.synchronize()
    assert bool(_is_sent(dst).all())
    assert lib.vitcap_copy_row_blocks(*args(g['cols'])) == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    want = torch.full((g['B'], g['dst_img_rows'], g['ld_dst']), SENT16, dtype=torch.int16)
    blk = _bits(src).view(g['B'], g['src_img_rows'], g['ld_src'])[:, g['src_row0']:g['src_row0'] + g['rows'],
                                                                  g['src_col0']:g['src_col0'] + g['cols']]
    want[:, g['dst_row0']:g['dst_row0'] + g['rows'], g['dst_col0']:g['dst_col0'] + g['cols']] = blk
    assert torch.equal(_bits(dst).view_as(want), want)
    assert torch.equal(_bits(src_d), _bits(src))


@pytest.mark.parametrize('n_tok', [577, 5])
def test_assemble_visual(lib, n_tok):
    """vis[b] = [tag_hidden[b, 0], hidden[b, 0 .. n_tok-1]] (modeling_bert.py:1493): fp32 copy exact, bf16 copy = RNE of it."""
    B = 3
    hidden = _rand((B, n_tok, 768), 171, 3.0)
    tag_hidden = _rand((B, n_tok, 768), 172, 3.0)
    vf, vb = _sent_f32(B, n_tok + 1, 768), _sent_bf16(B, n_tok + 1, 768)
    hid_d, tag_d = hidden.cuda(), tag_hidden.cuda()
    assert lib.vitcap_assemble_visual(_p(hid_d), _p(tag_d), _p(vf), _p(vb), B, n_tok, _s()) == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    want = torch.cat([tag_hidden[:, :1], hidden], 1)
    assert torch.equal(_bits(vf), _bits(want))
    assert torch.equal(_bits(vb), _bits(want.bfloat16()))


@pytest.mark.parametrize('D', [768, 1000])
def test_gather_rows_bf16(lib, D):
    """out[b] = bf16(x[b][0]) for x [B][ldx_rows][D]; D = 1000: the 256 threads loop four times, the last trip partly"""
    B, ldx_rows = 3, 7
    x = _rand((B, ldx_rows, D), 173, 3.0)
    x_d, out = x.cuda(), _sent_bf16(B + 1, D)
    assert lib.vitcap_gather_rows_bf16(_p(x_d), ldx_rows, _p(out), B, D, _s()) == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[:B]), _bits(x[:, 0].bfloat16()))
    assert bool(_is_sent(out[B:]).all())


# ------------------------------------------------------------------------------------------------ f. training small ops
@pytest.fixture(scope='module')
def emb(sd_t):
    e = 'module.bert.embeddings'
    word = _bf(sd_t[e + '.word_embeddings.weight'])
    pos = _bf(sd_t[e + '.position_embeddings.weight'])
    typ = _bf(sd_t[e + '.token_type_embeddings.weight'])
    g, b = sd_t[e + '.LayerNorm.weight'].float(), sd_t[e + '.LayerNorm.bias'].float()
    return dict(word=word, pos=pos, typ=typ, g=g, b=b, dev=[x.cuda().contiguous() for x in (word, pos, typ, g, b)])


def _positions(rows, rows_per_seq, pos_wrap):
    """position id of every row: r, or r - pos_wrap + 1 for the [MASK] probe rows r >= pos_wrap"""
    r = torch.arange(rows) % rows_per_seq
    return torch.where(r >= pos_wrap, r - pos_wrap + 1, r) if pos_wrap > 0 else r


# rows = 3 * 39 = 117 is no multiple of the 4 rows per workgroup: the last workgroup is partial
EMBED_GEOM = [(39, 20), (20, 0)]


@pytest.mark.parametrize('rows_per_seq,pos_wrap', EMBED_GEOM)
def test_embed_rows(lib, emb, rows_per_seq, pos_wrap):
    """BertEmbeddings.forward on every row of the teacher-forced caption (+ the [MASK] probe rows at positions r - pos_wrap + 1):
    the pre-LayerNorm sum is exactly (word + pos) + type in fp32; the LayerNorm outputs against an fp64 LayerNorm with
    test_embed_step's tolerance (the same ln_row); with pre_f32 = NULL the other outputs do not change."""
    rows = 3 * rows_per_seq
    ids = torch.randint(0, 30522, (rows,), generator=torch.Generator().manual_seed(180))
    pos_id = _positions(rows, rows_per_seq, pos_wrap)
    if pos_wrap:
        assert pos_id[20:39].tolist() == list(range(1, 20))
        ids[(torch.arange(rows) % rows_per_seq) >= pos_wrap] = 103
    word, pos, typ, g, b = emb['dev']
    ids_d = ids.cuda()
    outs = []
    for with_pre in (True, False):
        pre = _sent_f32(rows + 1, 768) if with_pre else None
        xf, xb = _sent_f32(rows + 1, 768), _sent_bf16(rows + 1, 768)
        assert lib.vitcap_embed_rows(_p(ids_d), rows_per_seq, _p(word), _p(pos), _p(typ), _p(g), _p(b), 1e-12, _p(pre), _p(xf), _p(xb),
                                     rows, pos_wrap, _s()) == 0, lib.vitcap_last_error()
        torch.cuda.synchronize()
        outs.append((pre, xf, xb))
    pre, xf, xb = outs[0]
    want_pre = (emb['word'].float()[ids] + emb['pos'].float()[pos_id]) + emb['typ'].float()[0]
    assert torch.equal(_bits(pre[:rows]), _bits(want_pre))
    want = torch.nn.functional.layer_norm(want_pre.double(), (768,), emb['g'].double(), emb['b'].double(), 1e-12)
    _close(xf[:rows], want, 1e-5, 1e-5, 'embed_rows LayerNorm (rows_per_seq %d, pos_wrap %d)' % (rows_per_seq, pos_wrap))
    assert torch.equal(_bits(xb[:rows]), _bits(xf[:rows].cpu().bfloat16()))
    for t in (pre, xf, xb):
        assert bool(_is_sent(t[rows:]).all())
    assert torch.equal(_bits(outs[1][1]), _bits(xf)) and torch.equal(_bits(outs[1][2]), _bits(xb))


@pytest.mark.parametrize('rows_per_seq,pos_wrap', EMBED_GEOM)
def test_embed_bwd(lib, rows_per_seq, pos_wrap):
    """BertEmbeddings backward: gword[ids[r]] += d[r], gpos[pos(r)] += d[r], gtype[0] += d[r] into tables that already hold
    something (the contract is +=), with [MASK] on every probe row, tokens repeated within and across sequences, and pos_wrap
    folding slots p and p + 19 onto one position row.  Reference: fp64 index_add.  The fp32 atomics may land in any order, so
    the bound is the any-order summation bound per element, n_i * 2^-24 * sum |terms_i| with n_i = the number of d rows added to
    element i and terms_i = those values and the value the table held (which is one of the numbers being summed); rtol = 0.
    Elements that nothing lands on (n_i = 0) must keep their bits."""
    n_seq, VW, NP = 3, 200, 40
    rows = n_seq * rows_per_seq
    gen = torch.Generator().manual_seed(181)
    d = _rand((rows, 768), 182)
    ids = torch.randint(0, VW, (rows,), generator=gen)
    slot = torch.arange(rows) % rows_per_seq
    ids[slot == 1] = 7                                  # the same token in every sequence
    ids[(slot == 2) | (slot == 3)] = 11                 # and twice within each
    if pos_wrap:
        ids[slot >= pos_wrap] = 103                     # [MASK] on every probe row: 19 x 3 rows onto one table row
    pos_id = _positions(rows, rows_per_seq, pos_wrap)
    init = [_rand((VW, 768), 183, 0.5) + 0.75, _rand((NP, 768), 184, 0.5) - 0.75, _rand((2, 768), 185, 0.5) + 0.75]
    dev = [x.cuda().contiguous() for x in init]
    d_d, ids_d = d.cuda(), ids.cuda()
    assert lib.vitcap_embed_bwd(_p(d_d), _p(ids_d), rows_per_seq, _p(dev[0]), _p(dev[1]), _p(dev[2]), rows, pos_wrap, _s()) == 0, \
        lib.vitcap_last_error()
    torch.cuda.synchronize()
    typ_id = torch.zeros(rows, dtype=torch.long)
    for name, got, g0, index in (('gword', dev[0], init[0], ids), ('gpos', dev[1], init[1], pos_id), ('gtype', dev[2], init[2], typ_id)):
        want = g0.double().index_add(0, index, d.double())
        n = torch.zeros(g0.shape[0]).index_add(0, index, torch.ones(rows))
        mag = g0.double().abs().index_add(0, index, d.double().abs())
        atol = n[:, None].double() * 2.0 ** -24 * mag
        err = (got.cpu().double() - want).abs()
        hit = n > 0
        _report('embed_bwd %s (rows_per_seq %d, pos_wrap %d)' % (name, rows_per_seq, pos_wrap), err[hit], atol[hit])
        assert bool((err <= atol).all()), '%s: %d elements off, max err %.3e' % (name, int((err > atol).sum()), float(err.max()))
        assert torch.equal(_bits(got.cpu()[~hit]), _bits(g0[~hit])) and int((~hit).sum()) > 0, name
    if pos_wrap:
        assert int(torch.bincount(pos_id)[1]) == 2 * n_seq and int(torch.bincount(ids)[103]) >= 19 * n_seq


def test_embed_bwd_rejects_partial_sequence(lib):
    d = torch.zeros(40, 768, device='cuda')
    ids = torch.zeros(40, dtype=torch.int64, device='cuda')
    tabs = [_sent_f32(4, 768) for _ in range(3)]
    _refused(lib, lib.vitcap_embed_bwd(_p(d), _p(ids), 39, _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), 40, 20, _s()), b'embed_bwd')
    torch.cuda.synchronize()
    assert all(bool(_is_sent(t).all()) for t in tabs)


def test_gelu_bwd(lib):
    """dz = bf16(dg * f) bit for bit, n = 1000 (the last 256-thread workgroup is partial); nothing behind n is written"""
    n = 1000
    dg = _rand((n,), 190, 3.0)
    f = _bf(_rand((n,), 191, 1.2))
    dg_d, f_d, dz = dg.cuda(), f.cuda(), _sent_bf16(n + 24)
    assert lib.vitcap_gelu_bwd(_p(dg_d), _p(f_d), _p(dz), n, _s()) == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(dz[:n]), _bits((dg * f.float()).bfloat16()))
    assert bool(_is_sent(dz[n:]).all())


def test_sum_over_batch(lib):
    """out[j] = ((((0 + x[0][j]) + x[1][j]) + ...) + x[B-1][j]) in fp32, bit for bit, rows `stride` > n apart"""
    B, n, stride = 5, 1000, 1536
    x = _rand((B, stride), 192, 3.0)
    x_d, out = x.cuda(), _sent_f32(n + 24)
    assert lib.vitcap_sum_over_batch(_p(x_d), stride, B, _p(out), n, _s()) == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    want = torch.zeros(n)
    for b in range(B):
        want = want + x[b, :n]
    assert torch.equal(_bits(out[:n]), _bits(want))
    assert bool(_is_sent(out[n:]).all())


@pytest.mark.parametrize('M,rows_per_seq,row0', [(2 * 20, 20, 578), (2 * 598, 598, 0)], ids=['text_rows_at_578', 'joint_rows'])
@pytest.mark.parametrize('p', [0.0, 0.1, 0.5])
def test_hidden_dropout(ops, lib, p, M, rows_per_seq, row0):
    """vitcap_hidden_dropout on its own: the keep mask is oracle.hidden_keep's for rows row0 .. row0 + rows_per_seq - 1 of every
    sequence (exactly: the zeros of the run without residual are the oracle's dropped positions), kept values are
    x / (1 - p) (+ residual), and the same call on a gradient with the same seed draws the same mask (the backward use).
    Bound on a kept value: the kernel multiplies by the fp32 scale s = fl(1 / fl(1 - p)) -- fl(x * s) is within 2^-24 (s) + 2^-24
    (the product's rounding) = 2^-23 relative, one fp32 ulp, of x / (1 - p) -- and then adds the residual (one more rounding of the
    sum, 2^-24 relative to it; a fused multiply-add only drops the product's rounding):
    |err| <= 2^-23 |x / (1 - p)| + 2^-24 |x / (1 - p) + residual|, times (1 + 2^-20) for the second-order terms."""
    from oracle import vitcap_oracle as O
    seed, B = 0xC0FFEE + int(p * 10), M // rows_per_seq
    x = _rand((M, 768), 193)
    x = torch.where(x >= 0, x + 0.25, x - 0.25)                   # no zeros: a zero in the output is a dropped position
    res = _rand((M, 768), 194, 2.0)
    dy = torch.where(res >= 0, res + 0.25, res - 0.25)
    keep = torch.from_numpy(O.hidden_keep(seed, B, p, rows=598)[:, row0:row0 + rows_per_seq].reshape(M, 768))
    if p == 0.0:
        assert bool(keep.all())
    else:
        assert abs(float(keep.float().mean()) - (1 - p)) < 0.02
    xd = x.cuda()
    plain = ops.hidden_dropout(xd, None, rows_per_seq, row0, seed, p)
    fused = ops.hidden_dropout(xd, res.cuda(), rows_per_seq, row0, seed, p)
    back = ops.hidden_dropout(dy.cuda(), None, rows_per_seq, row0, seed, p)
    torch.cuda.synchronize()
    assert torch.equal(plain.cpu() != 0, keep), 'dropped positions differ from oracle.hidden_keep'
    assert torch.equal(back.cpu() != 0, keep), 'the backward call drew another mask'
    q = float(np.float32(1.0) - np.float32(p))                    # the kernel's fp32 1 - p
    a = torch.where(keep, x.double() / q, torch.zeros((), dtype=torch.float64))
    slack = 1 + 2.0 ** -20
    for what, got, want in (('no residual', plain, a), ('residual', fused, a + res.double()),
                            ('gradient', back, torch.where(keep, dy.double() / q, torch.zeros((), dtype=torch.float64)))):
        base = a if what != 'gradient' else want
        tol = (2.0 ** -23 * base.abs() + (2.0 ** -24 * want.abs() if what == 'residual' else 0.0)) * slack
        err = (got.cpu().double() - want).abs()
        _report('hidden_dropout p=%g %s M=%d' % (p, what, M), err, tol + 1e-300)
        assert bool((err <= tol).all()), '%s: max err %.3e' % (what, float(err.max()))
    assert torch.equal(_bits(xd), _bits(x))


def test_hidden_dropout_rejects_p_one(lib):
    x = torch.ones(4, 768, device='cuda')
    out = _sent_f32(4, 768)
    _refused(lib, lib.vitcap_hidden_dropout(_p(x), None, _p(out), 4, 768, 4, 0, 1, 1.0, _s()), b'hidden_dropout')
    torch.cuda.synchronize()
    assert bool(_is_sent(out).all())


# ------------------------------------------------------------------------------------------------ g. decode bookkeeping reached only through the engine
def test_repetition_penalty(lib):
    """CTRL penalty kernel alone (modeling_utils.py:828-836): every DISTINCT token of ids[row][:t] has its logit divided by the
    penalty if positive, multiplied if negative -- once, however often it repeats; tokens at positions >= t and ids outside
    [0, V) leave the row alone.  One fp32 multiply or divide per element: bit for bit.  6 rows: the second workgroup is partial."""
    rows, V, ldl, ld_ids, t, pen = 6, 30522, 30592, 20, 7, 1.3
    logits = _rand((rows, ldl), 200, 4.0)
    ids = torch.randint(0, V, (rows, ld_ids), generator=torch.Generator().manual_seed(201))
    ids[0, 1] = ids[0, 4] = ids[0, 6] = 777            # repeats inside the prefix: penalised once
    ids[1, 2] = ids[1, 9]                              # a repeat whose second occurrence lies behind t
    ids[2, 3] = V + 5                                  # a padding column: not a token
    ids[3, :t] = torch.arange(100, 100 + t)
    logits[3, 100:100 + t] = torch.tensor([2.0, -2.0, 0.0, -0.0, 1e-30, -1e30, 5.5])
    logits_d, ids_d = logits.cuda(), ids.cuda()
    assert lib.vitcap_repetition_penalty(_p(logits_d), ldl, V, _p(ids_d), ld_ids, t, pen, rows, _s()) == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    want = logits.clone()
    p32 = torch.tensor(pen, dtype=torch.float32)
    for r in range(rows):
        for tok in sorted(set(int(x) for x in ids[r, :t] if 0 <= int(x) < V)):
            v = logits[r, tok]
            want[r, tok] = v * p32 if v < 0 else v / p32
    assert int((want != logits).sum()) >= rows * (t - 2)
    assert torch.equal(_bits(logits_d), _bits(want))
    _refused(lib, lib.vitcap_repetition_penalty(_p(logits_d), ldl, V, _p(ids_d), ld_ids, ld_ids + 1, pen, rows, _s()), b'repetition_penalty')


def test_sample_step_offset_draws_the_whole_batch_rows(ops, lib):
    """vitcap_sample_step_offset: rows that are sequences seq_offset .. of a larger call draw from THEIR random streams.  A batch of
    6 cut into two slices of 3 (offsets 0 and 3) must pick, row for row, the tokens the CPU sampler (oracle.make_sampler, stream =
    (seed, sequence, t)) picks for the whole batch; the Gumbel-argmax margins of these rows are > 0.1, far above fp32 noise."""
    from oracle import vitcap_oracle as O
    from vitcap_amd._lib import SampleParams
    B, V, ld, t, seed = 6, 30522, 30592, 3, 99
    logits = torch.randn(B, ld, generator=torch.Generator().manual_seed(21)) * 2
    tok, lp, margin = O.make_sampler(1.0, 0, 1.0, seed=seed)(logits[:, :V].contiguous(), t)
    assert float(margin.min()) > 0.1
    logits_d = logits.cuda()
    sp = SampleParams(1, 1.0, 0, 1.0, seed)
    for off in (0, 3):
        st = ops.greedy_init(3)
        sl = logits_d[off:off + 3]
        assert lib.vitcap_sample_step_offset(_p(sl), ld, V, _p(st['ids']), _p(st['unf']), _p(st['sum_lp']), _p(st['cnt']), _p(st['logprob']),
                                             _p(st['margin']), None, 3, t, 20, 102, 0, C.byref(sp), off, _s()) == 0, lib.vitcap_last_error()
        torch.cuda.synchronize()
        assert st['ids'][:, t].cpu().tolist() == tok[off:off + 3].tolist(), off
        _close(st['sum_lp'], lp[off:off + 3], 1e-5, 1e-5, 'sample_step_offset log-prob (offset %d)' % off)
