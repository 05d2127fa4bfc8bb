"""Per-element parity of the training attention kernels (attn_dense_kernel in its training form, attn_bwd_dq_dma_kernel,
attn_bwd_dkv_dma_kernel) with an fp64 reference at tile, mask, probe and query-range edges (docs/LAB_tests_attn_train_edges.md).

Each case runs the forward and then the backward on the kernel's OWN out / lse, and compares out, lse, dQ, dK, dV element by
element with oracle/attn_train_ref.reference under bounds derived from the kernels' rounding points; no aggregate norm anywhere.
The inputs are planted (a query's softmax sits on one chosen key), so that one wrong (query, key) decision moves a row by many
bounds: tests/test_attn_train_edges_cpu.py proves that for every mutation of the rule, without a GPU.  Every buffer the kernels
write is pre-filled with the sentinel bf16 0x7B7B / fp32 0x7B7B7B7B, which must survive wherever the contract says "not written";
rows S..ld_rows of the inputs hold NaN, so a read of them shows.  Each comparison prints its largest error / bound (`pytest -s`).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import attn_train_ref as R

pytestmark = pytest.mark.gpu

SENT16 = 0x7B7B
SENT32 = 0x7B7B7B7B
SCALE = 0.125


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vitcap_amd._lib import lib as l
    return l


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sent_bf16(*shape):
    return torch.full(shape, SENT16, dtype=torch.int16, device='cuda').view(torch.bfloat16)


def _sent_f32(*shape):
    return torch.full(shape, SENT32, dtype=torch.int32, device='cuda').view(torch.float32)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _all_sent(t):
    b = _bits(t)
    return bool((b == (SENT16 if b.dtype == torch.int16 else SENT32)).all())


def _padded(t, ld):
    """(B, S, D) bf16 -> device (B, ld, D) with NaN in the rows S..ld that no kernel may read."""
    B, S, D = t.shape
    buf = torch.full((B, ld, D), float('nan'), dtype=torch.bfloat16)
    buf[:, :S] = t
    return buf.cuda().contiguous()


def _run(lib, case, qkv, dout, extra=None, forwarders=False, mf=None):
    """Forward, then the backward on the forward's own out / lse.  Returns the raw buffers (out (B, ld, 768), lse (B, 12, S),
    dqkv (B, ld, 2304), dsum) on the CPU.  forwarders: through vitcap_attn_dense_fwd_train / vitcap_attn_dense_bwd."""
    B, S, ld, cf, mf_case, p, qr = case
    mf = mf_case if mf is None else mf
    lo, hi = (0, S) if qr is None else qr
    qd, dd = _padded(qkv, ld), _padded(dout, ld)
    ed = _padded(extra, ld) if extra is not None else None
    out, lse = _sent_bf16(B, ld, 768), _sent_f32(B, 12, S)
    dqkv, dsum = _sent_bf16(B, ld, 2304), _sent_f32(B, 12, S)
    if forwarders:
        assert qr is None
        rc = lib.vitcap_attn_dense_fwd_train(_p(qd), _p(out), _p(lse), B, S, ld, SCALE, p, R.DROP_SEED, cf, mf, _s())
        assert rc == 0, lib.vitcap_last_error()
        rc = lib.vitcap_attn_dense_bwd(_p(qd), _p(out), _p(dd), _p(lse), _p(dsum), _p(ed), _p(dqkv), B, S, ld, SCALE, p, R.DROP_SEED,
                                       cf, mf, _s())
        assert rc == 0, lib.vitcap_last_error()
    else:
        rc = lib.vitcap_attn_dense_fwd_train_rows(_p(qd), _p(out), _p(lse), B, S, ld, SCALE, p, R.DROP_SEED, cf, mf, lo, hi, _s())
        assert rc == 0, lib.vitcap_last_error()
        rc = lib.vitcap_attn_dense_bwd_rows(_p(qd), _p(out), _p(dd), _p(lse), _p(dsum), _p(ed), _p(dqkv), B, S, ld, SCALE, p,
                                            R.DROP_SEED, cf, mf, lo, hi, _s())
        assert rc == 0, lib.vitcap_last_error()
    torch.cuda.synchronize()
    return dict(out=out.cpu(), lse=lse.cpu(), dqkv=dqkv.cpu(), dsum=dsum.cpu())


@functools.lru_cache(maxsize=None)
def _inputs(case):
    return R.case_inputs(case)


@functools.lru_cache(maxsize=None)
def _reference(case, with_extra=False):
    B, S, ld, cf, mf, p, qr = case
    qkv, dout, keep = _inputs(case)
    extra = R._rand((B, S, 1536), 77 + S, 1.0).to(torch.bfloat16) if with_extra else None
    return R.reference(qkv, dout, R.visible(S, cf, mf), keep, p, SCALE, extra=extra), extra


def _within(what, got, want, bound):
    """|got - want| <= bound at every element (a NaN or a left-over sentinel is off); prints where the largest err/bound sits."""
    got = got.double()
    err = (got - want).abs()
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float('inf')), ratio)
    i = int(ratio.flatten().argmax())
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape)))
    print('MEASURED %s: largest err/bound %.3f at %s (err %.3e, bound %.3e, want %.3e)' % (
        what, float(ratio.flatten()[i]), idx, float(err.flatten()[i]), float(bound.flatten()[i]), float(want.flatten()[i])))
    bad = ~(err <= bound)
    assert not bad.any(), '%s: %d/%d elements beyond their bound, largest err/bound %.3g at %s, first %s' % (
        what, int(bad.sum()), bad.numel(), float(ratio.flatten()[i]), idx, bad.nonzero()[:4].tolist())


def _check(case, got, ref):
    """All five tensors against the reference, and the sentinel wherever nothing may be written."""
    B, S, ld, cf, mf, p, qr = case
    lo, hi = R.covered_rows(S, qr)          # the 128-row blocks of the query range
    name = R.case_id(case)
    out, lse, dqkv = got['out'], got['lse'], got['dqkv']
    _within(name + ' out', out[:, lo:hi], ref['out'][:, lo:hi], ref['b_out'][:, lo:hi])
    _within(name + ' lse', lse[:, :, lo:hi], ref['lse2'][:, :, lo:hi], R.lse_bound(ref['lse2'])[:, :, lo:hi])
    _within(name + ' dq', dqkv[:, lo:hi, :768], ref['dq'][:, lo:hi], ref['b_dq'][:, lo:hi])
    _within(name + ' dk', dqkv[:, :S, 768:1536], ref['dk'], ref['b_dk'])
    _within(name + ' dv', dqkv[:, :S, 1536:], ref['dv'], ref['b_dv'])
    assert _all_sent(out[:, S:]) and _all_sent(dqkv[:, S:]), 'rows S..ld_rows were written'
    assert _all_sent(out[:, :lo]) and _all_sent(out[:, hi:S]), 'forward rows outside the blocks of the range were written'
    assert _all_sent(lse[:, :, :lo]) and _all_sent(lse[:, :, hi:]), 'lse outside the blocks of the range was written'
    assert _all_sent(dqkv[:, :lo, :768]) and _all_sent(dqkv[:, hi:S, :768]), 'dQ rows outside the blocks of the range were written'
    assert not bool(((_bits(dqkv[:, :S, 768:]) == SENT16).all(-1)).any()), 'a key row of dK / dV was not written'


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_forward_backward_per_element(lib, case):
    B, S, ld, cf, mf, p, qr = case
    qkv, dout, keep = _inputs(case)
    ref, _ = _reference(case)
    got = _run(lib, case, qkv, dout)
    _check(case, got, ref)
    if cf == S:                              # no caption rows: the reference it met is the unmasked one
        assert bool(R.visible(S, cf, mf).all())
    if cf > 0 and mf == S:                   # no probe rows: the same bits as without mask_from
        plain = _run(lib, case, qkv, dout, mf=0)
        for n in ('out', 'lse', 'dqkv'):
            assert torch.equal(_bits(got[n]), _bits(plain[n])), n


@pytest.mark.parametrize('case', [(2, 72, 80, 0, 0, 0.0, None), (2, 598, 598, 578, 0, 0.0, None)], ids=R.case_id)
def test_extra_dkv(lib, case):
    """extra_dkv (B * ld_rows, 1536) = [dK | dV] is added to dK / dV before their one rounding; dQ and the forward do not move."""
    B, S, ld, cf, mf, p, qr = case
    assert case in R.CASES
    qkv, dout, keep = _inputs(case)
    ref, extra = _reference(case, True)
    got = _run(lib, case, qkv, dout, extra=extra)
    _check(case, got, ref)
    plain = _run(lib, case, qkv, dout)
    assert torch.equal(_bits(got['dqkv'][:, :S, :768]), _bits(plain['dqkv'][:, :S, :768]))
    assert not torch.equal(_bits(got['dqkv'][:, :S, 768:]), _bits(plain['dqkv'][:, :S, 768:]))


@pytest.mark.parametrize('case', [(2, 73, 73, 0, 0, 0.0, None), (2, 617, 617, 578, 598, 0.1, None)], ids=R.case_id)
def test_forwarders_equal_whole_range(lib, case):
    """vitcap_attn_dense_fwd_train / vitcap_attn_dense_bwd are the _rows entry points with the range [0, S): the same bits."""
    assert case in R.CASES
    qkv, dout, keep = _inputs(case)
    a = _run(lib, case, qkv, dout, forwarders=True)
    b = _run(lib, case, qkv, dout)
    for n in ('out', 'lse', 'dqkv', 'dsum'):
        assert torch.equal(_bits(a[n]), _bits(b[n])), n
    assert not _all_sent(a['dqkv'][:, :case[1]])


REFUSED = [    # (why, S, ld_rows, cf, mf, q_lo, q_hi, p_drop)
    ('causal_from below the last key tile', 640, 640, 578, 0, 0, 640, 0.0),
    ('causal_from > S', 598, 598, 599, 0, 0, 598, 0.0),
    ('mask_from <= causal_from', 617, 617, 578, 578, 0, 617, 0.0),
    ('mask_from > S', 617, 617, 578, 618, 0, 617, 0.0),
    ('mask_from without causal_from', 617, 617, 0, 598, 0, 617, 0.0),
    ('q_lo = 64', 598, 598, 578, 0, 64, 598, 0.0),
    ('q_hi > S', 598, 598, 578, 0, 0, 599, 0.0),
    ('ld_rows < S', 598, 597, 578, 0, 0, 598, 0.0),
    ('ld_rows = 1024', 598, 1024, 578, 0, 0, 598, 0.0),
    ('p_drop = 1', 598, 598, 578, 0, 0, 598, 1.0),
]


@pytest.mark.parametrize('why,S,ld,cf,mf,lo,hi,p', REFUSED, ids=[r[0].replace(' ', '_') for r in REFUSED])
def test_refused_without_a_launch(lib, why, S, ld, cf, mf, lo, hi, p):
    """Outside the contract both entry points return an error and launch nothing: every output keeps the sentinel."""
    rows = max(S, ld) + 1
    qd = torch.zeros(rows, 2304, dtype=torch.bfloat16, device='cuda')
    dd = torch.zeros(rows, 768, dtype=torch.bfloat16, device='cuda')
    out, lse = _sent_bf16(rows, 768), _sent_f32(12, rows)
    dqkv, dsum = _sent_bf16(rows, 2304), _sent_f32(12, rows)
    rc = lib.vitcap_attn_dense_fwd_train_rows(_p(qd), _p(out), _p(lse), 1, S, ld, SCALE, p, 1, cf, mf, lo, hi, _s())
    assert rc != 0 and b'attn_dense_train' in lib.vitcap_last_error(), why
    fwd_out = torch.zeros(rows, 768, dtype=torch.bfloat16, device='cuda')
    fwd_lse = torch.zeros(12, rows, dtype=torch.float32, device='cuda')
    rc = lib.vitcap_attn_dense_bwd_rows(_p(qd), _p(fwd_out), _p(dd), _p(fwd_lse), _p(dsum), None, _p(dqkv), 1, S, ld, SCALE, p, 1,
                                        cf, mf, lo, hi, _s())
    assert rc != 0 and b'attn_dense_bwd' in lib.vitcap_last_error(), why
    torch.cuda.synchronize()
    assert _all_sent(out) and _all_sent(lse) and _all_sent(dqkv) and _all_sent(dsum), why
