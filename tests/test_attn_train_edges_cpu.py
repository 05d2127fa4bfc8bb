"""Teeth of tests/test_hip_attn_train_edges.py, checked without a GPU and without a kernel (docs/LAB_tests_attn_train_edges.md).

The GPU test compares the training attention kernels with oracle/attn_train_ref.reference element by element under derived
bounds.  A kernel with one wrong visibility decision sits within one bound of the equally wrong reference, so it is certain to
fail only where the right and the wrong reference are more than two bounds apart.  This file requires 2.5 bounds, for every
masked case of the table and every mutation that applies to it, in each of the three kernels' outputs: a condition on the
planted inputs, not a measurement of anything.
"""
import pytest
import torch

from oracle import attn_train_ref as R

FACTOR = 2.5
PLANTED = [0, 1, 2, 3, 4, 5, 6]          # the heads planted_inputs builds: the largest distance over a subset is a lower bound
MASKED = [c for c in R.CASES if c[3] > 0]


def _joint_visible(q, k, S, cf, mf):
    """vitcap_amd/csrc/common.h joint_visible, line by line."""
    plain = cf <= 0 or k < cf
    causal = k <= q
    probe_q = mf > 0 and q >= mf
    probe_k = mf > 0 and k >= mf
    text = (k == q) if probe_k else (((k - cf) <= (q - mf)) if probe_q else causal)
    return k < S and (plain or text)


@pytest.mark.parametrize('S,cf,mf', [(40, 10, 25), (23, 17, 0), (9, 0, 0), (12, 5, 12)])
def test_visible_is_the_kernels_rule(S, cf, mf):
    want = torch.tensor([[_joint_visible(q, k, S, cf, mf) for k in range(S)] for q in range(S)])
    assert torch.equal(R.visible(S, cf, mf), want)
    if cf > 0 and cf < mf < S:            # with all three kinds of row present every mutation is a different rule somewhere
        for m in R.MASK_MUTATIONS:
            assert not torch.equal(R.visible(S, cf, mf, m).long(), want.long()), m


def _mutations(case, mask):
    """The mutations that apply to a case: a mask mutation when it changes the visibility of some key for a query row INSIDE the
    query range (rows outside carry no dout and their forward rows are not part of the range's contract, so nothing the three
    kernels return could show it); image-1 with two images or more; the dropout mutations with p > 0."""
    B, S, ld, cf, mf, p, qr = case
    lo, hi = (0, S) if qr is None else qr
    muts = [m for m in R.MASK_MUTATIONS if not torch.equal(R.visible(S, cf, mf, m)[lo:hi].long(), mask[lo:hi].long())]
    return muts + (['image-1'] if B >= 2 else []) + (['drop-shift', 'drop-T'] if p > 0 else [])


def _ratio(wrong, right, name, rows):
    """Largest |wrong - right| / bound over the compared rows; an element that moves where the bound is zero counts as infinite."""
    d = (wrong[name] - right[name]).abs()[:, rows]
    b = right['b_' + name][:, rows]
    r = torch.where(d > 0, d / b, torch.zeros_like(d))
    return float(r.max())


@pytest.mark.parametrize('case', MASKED, ids=R.case_id)
def test_no_mutation_hides(case):
    B, S, ld, cf, mf, p, qr = case
    qkv, dout, keep = R.case_inputs(case)
    mask = R.visible(S, cf, mf)
    right = R.reference(qkv, dout, mask, keep, p, heads=PLANTED)
    lo, hi = R.covered_rows(S, qr)
    muts = _mutations(case, mask)
    assert 'lastkey' in muts and 'pastend' in muts and ('diag' in muts or cf == S)
    short = []
    for m in muts:
        if m in R.MASK_MUTATIONS:
            wrong = R.reference(qkv, dout, R.visible(S, cf, mf, m), keep, p, heads=PLANTED)
        else:
            qkv_m, keep_m = R.mutate_data(qkv, keep, m)
            wrong = R.reference(qkv_m, dout, mask, keep_m, p, heads=PLANTED)
        fwd = _ratio(wrong, right, 'out', slice(lo, hi))
        dq = _ratio(wrong, right, 'dq', slice(lo, hi))
        dkv = max(_ratio(wrong, right, 'dk', slice(0, S)), _ratio(wrong, right, 'dv', slice(0, S)))
        print('TEETH %s %-11s out %.3g dq %.3g dk|dv %.3g' % (R.case_id(case), m, fwd, dq, dkv))
        if min(fwd, dq, dkv) < FACTOR:
            short.append((m, fwd, dq, dkv))
    assert not short, 'mutations within %.1f bounds of the right reference (out, dq, dk|dv): %s' % (FACTOR, short)


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_bounds_leave_room_for_the_rounding_they_count(case):
    """The bounds are derived from the kernels' rounding points; arithmetic with exactly those rounding points (emulate: fp64 in
    between) must therefore sit inside them, lse2 included.  Shows a missing term without spending a GPU run on it."""
    B, S, ld, cf, mf, p, qr = case
    qkv, dout, keep = R.case_inputs(case)
    mask = R.visible(S, cf, mf)
    heads = PLANTED + [11]
    ref = R.reference(qkv, dout, mask, keep, p, heads=heads)
    emu = R.emulate(qkv, dout, mask, keep, p, heads=heads)
    lo, hi = R.covered_rows(S, qr)
    for n in ('out', 'dq', 'dk', 'dv'):
        rows = slice(lo, hi) if n in ('out', 'dq') else slice(0, S)
        assert bool(((emu[n] - ref[n]).abs()[:, rows] <= ref['b_' + n][:, rows]).all()), n
    assert bool(((emu['lse2'] - ref['lse2']).abs() <= R.lse_bound(ref['lse2'])).all())
