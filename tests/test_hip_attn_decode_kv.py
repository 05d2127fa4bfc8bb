"""Decode attention with the visual K/V streamed apart from the other keys (vitcap_amd/csrc/attn.hip, attn_decode_kernel and
attn_decode_beam_kernel): the sweeps that hold visual keys only go through a buffer descriptor with the non-temporal policy, the
sweep the visual rows end in and the keys behind it (text cache, this step's rows) through generic loads.

Shapes are the smallest at which that split can go wrong: S_vis below one 32-key slot, one key either side of a slot (31, 33)
and of a 128-key sweep (127, 129), exactly one and two sweeps (128, 256: no visual key left for the mixed sweep) and the real
578 (four whole sweeps, 66 visual keys sharing the fifth with the text keys).  Except at 128 and 256 the visual / text boundary
falls inside a sweep.

Reference and tolerance are those of tests/test_hip_ops.py::test_attn_decode_step: fp32 on the same bf16 operands with the
device's rounding points (oracle.softmax_pv_rounded), 2^-7 relative + 2e-3 absolute (fp32 summation order plus one bf16 rounding
of the output).  Run on the GPU box:  python -m pytest tests/test_hip_attn_decode_kv.py -m gpu -q
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

L = 20                       # text cache rows per sequence
RTOL, ATOL = 2 ** -7, 2e-3   # test_attn_decode_step's


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vitcap_amd import ops as o
    return o


def _bf(t):
    return t.to(torch.bfloat16)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _close(got, want, what):
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    err = (got - want).abs()
    bad = err > ATOL + RTOL * want.abs()
    assert not bad.any(), '%s: %d/%d elements off, max err %.3e (want max %.3e), first bad idx %s' % (
        what, int(bad.sum()), bad.numel(), float(err.max()), float(want.abs().max()), bad.nonzero()[:4].tolist())


def _n_seq(spi):
    """3 sequences; with two sequences per image the entry point wants whole images, so 4 (two images)."""
    return 3 if spi == 1 else 4


@functools.lru_cache(maxsize=None)
def _inputs(S, spi, B=None):
    """(visual q|k|v rows per image, text cache per sequence), made once per shape and never written to."""
    B = B or _n_seq(spi)
    vis = _bf(_rand((B // spi, S, 2304), 300 + S, 2.0))
    cache = _bf(_rand((B, L, 2, 768), 301 + S, 2.0))
    return vis, cache


def _step_rows(B, t):
    return _bf(_rand((B, 2, 2304), 310 + t, 2.0))


def _reference(vis, cache, step, t, spi):
    """keys = visual rows of the sequence's image | cached text 0..t-2 | this step's row 0 (position t-1) | [MASK] row"""
    from oracle import vitcap_oracle as O
    B = step.shape[0]
    visr = vis.repeat_interleave(spi, 0)
    K = torch.cat([visr[..., 768:1536].float(), cache[:, :t - 1, 0].float(), step[:, :, 768:1536].float()], 1)
    V = torch.cat([visr[..., 1536:].float(), cache[:, :t - 1, 1].float(), step[:, :, 1536:].float()], 1)
    q = step[..., :768].float().view(B, 2, 12, 64).transpose(1, 2)
    s = q @ K.view(B, -1, 12, 64).transpose(1, 2).transpose(-1, -2)
    s[:, :, 0, -1] = float('-inf')                        # row 0 (position t-1) does not see the [MASK] row
    return O.softmax_pv_rounded(s, V.view(B, -1, 12, 64).transpose(1, 2), O._R(True)).transpose(1, 2).reshape(B, 2, 768)


def _run(ops, vis, cache_dev, step, S, t, spi):
    B = step.shape[0]
    out = ops.attn_decode_step(step.reshape(B * 2, 2304).cuda().contiguous(), vis.reshape(-1, 2304).cuda().contiguous(), cache_dev,
                               B, S, t, max_len=L, seq_per_image=spi)
    torch.cuda.synchronize()
    return out.view(B, 2, 768)


@pytest.mark.parametrize('spi', [1, 2])
@pytest.mark.parametrize('t', [1, 2, 19])
@pytest.mark.parametrize('S', [1, 31, 33, 127, 128, 129, 256, 578])
def test_decode_step_parity(ops, S, t, spi):
    vis, cache = _inputs(S, spi)
    B = cache.shape[0]
    step = _step_rows(B, t)
    cache_dev = cache.cuda().contiguous()
    got = _run(ops, vis, cache_dev, step, S, t, spi)
    _close(got, _reference(vis, cache, step, t, spi), 'decode step S_vis=%d t=%d seq_per_image=%d' % (S, t, spi))
    # cache row t-1 now holds this step's real-token K/V, every other row is what it was
    c = cache_dev.cpu()
    assert torch.equal(c[:, t - 1, 0], step[:, 0, 768:1536]) and torch.equal(c[:, t - 1, 1], step[:, 0, 1536:])
    keep = [i for i in range(L) if i != t - 1]
    assert torch.equal(c[:, keep], cache[:, keep])


@pytest.mark.parametrize('S,t', [(129, 1), (578, 1), (33, 18), (578, 18)])
def test_decode_step_sees_the_row_the_step_before_published(ops, S, t):
    """Step t writes its real-token K/V into cache row t-1 with a plain store; step t+1, a later launch on the same cache, reads
    that row with a default-policy load and must see it.  The published key is made to matter: it is step t+1's [MASK] query
    itself, so its score (|q|^2 / 8, about 10) stands far above the others' (deviation about 2) and the row's output is close to
    the published V; the reference over the cache as it was before step t is then far from the one over the updated cache."""
    vis, cache = _inputs(S, 1)
    B = cache.shape[0]
    cache_dev = cache.cuda().contiguous()
    step_a, step_b = _step_rows(B, t).clone(), _step_rows(B, t + 1)
    step_a[:, 0, 768:1536] = step_b[:, 1, :768]
    want_cache = cache.clone()
    want_cache[:, t - 1, 0] = step_a[:, 0, 768:1536]
    want_cache[:, t - 1, 1] = step_a[:, 0, 1536:]
    want = _reference(vis, want_cache, step_b, t + 1, 1)
    stale = _reference(vis, cache, step_b, t + 1, 1)
    assert (want - stale).abs().max() > 0.5, 'the published row does not matter enough for this test to see it'
    _run(ops, vis, cache_dev, step_a, S, t, 1)
    got = _run(ops, vis, cache_dev, step_b, S, t + 1, 1)
    _close(got, want, 'step %d after step %d, S_vis=%d' % (t + 1, t, S))


@pytest.mark.parametrize('S,t', [(33, 2), (129, 19), (578, 19)])
def test_decode_step_deterministic_and_sliceable(ops, S, t):
    """Two runs give equal bits, and a 3-sequence batch equals its sequences run one at a time (one workgroup per (sequence,
    head): nothing in a sequence's result may depend on its neighbours)."""
    vis, cache = _inputs(S, 1)
    B = cache.shape[0]
    step = _step_rows(B, t)
    a = _run(ops, vis, cache.cuda().contiguous(), step, S, t, 1)
    b = _run(ops, vis, cache.cuda().contiguous(), step, S, t, 1)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    for i in range(B):
        one = _run(ops, vis[i:i + 1], cache[i:i + 1].cuda().contiguous(), step[i:i + 1], S, t, 1)
        assert torch.equal(one.view(torch.int16), a[i:i + 1].view(torch.int16)), 'sequence %d alone differs from the batch' % i


@pytest.mark.parametrize('S', [33, 578])
def test_decode_beams_vs_single_sequences(ops, S):
    """2 images x 3 beams on the matrix-pipe kernel (visual K rows and the V^T copy streamed non-temporally) against the
    per-sequence kernel, as test_attn_decode_beams_vs_single_sequences compares them: caches published identically, outputs within
    one bf16 ulp (same softmax and rounding points, another fp32 summation order); and against the fp32 reference."""
    n_img, K, t = 2, 3, 7
    B = n_img * K
    vis, cache = _inputs(S, K, B)
    step = _step_rows(B, t)
    c1, c2 = cache.cuda().contiguous(), cache.cuda().contiguous()
    step_d = step.reshape(B * 2, 2304).cuda().contiguous()
    vis_d = vis.reshape(n_img * S, 2304).cuda().contiguous()
    got = ops.attn_decode_beams(step_d, vis_d, c1, n_img, K, S, t, max_len=L)
    want = ops.attn_decode_step(step_d, vis_d, c2, B, S, t, max_len=L, seq_per_image=K)
    torch.cuda.synchronize()
    assert torch.equal(c1, c2)
    _close(got.view(B, 2, 768), want.view(B, 2, 768), 'beam attention vs per-sequence kernel S_vis=%d' % S)
    _close(got.view(B, 2, 768), _reference(vis, cache, step, t, K), 'beam attention vs reference S_vis=%d' % S)
