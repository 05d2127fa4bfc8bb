"""Test helper of the encoder-rollout tests (tests/test_rollout_cpu.py, tests/test_hip_rollout.py): fp64 restatements of the
self-attention probabilities vitcap_attn_self_maps defines (include/vitcap_hip.h), of one rollout step (vitcap_rollout_step) and of
the whole path vitcap_amd.rollout.rollout_rows walks, the inputs both suites feed them, the comparators and their bounds.  Pure
torch / numpy on the CPU; nothing here touches the GPU library.

Block order everywhere: blocks.0..11, then tag_blocks.0..3 (the engine's block_mask bits 0..15).  The model's graph
(modeling_bert.py:458-478): blocks 0..7, then the fork -- blocks 8..11 give the caption's 577 visual tokens, tag blocks 0..3 give the
tag branch, whose cls row is the 578th visual token (cache column 0) and the pooler's input."""
import os

import numpy as np
import torch

NH, HD, QKV_LD = 12, 64, 2304
NV, NVIS, NB, FORK = 577, 578, 16, 8
BLOCK_NAMES = tuple('blocks.%d' % i for i in range(12)) + tuple('tag_blocks.%d' % i for i in range(4))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_encattn.npz')

# |p - p_ref| <= OP_REL * p_ref + OP_ABS: the project's derived bound for this arithmetic (tests/attn_maps_ref.py): fp32 accumulation
# of a 64-term bf16 dot product, the 0.125 scale, and a row sum of at most 640 fp32 terms (620 there).
OP_REL, OP_ABS = 2e-4, 1e-7
# P.V rebuilt from the per-head rows against vitcap_attn_dense_fwd's bf16 output: the project's bound for that output.
PV_ABS, PV_REL = 2e-3, 2.0 ** -7
# One rollout step, every term nonnegative: 577 fused multiply-adds, the product with (1 - residual), its rounding and the final
# multiply-add -- at most 580 roundings of relative size 2^-24 each on a sum of nonnegative terms (Higham's gamma_n).
GAMMA = 580 * 2.0 ** -24 / (1.0 - 580 * 2.0 ** -24)
STEP_ABS = 1e-30
PATH_STEPS = 12          # 4 + 8 steps from either end of the fork to the encoder's input


def step_rel(n_steps):
    return (1.0 + GAMMA) ** n_steps - 1.0


# End to end against the reference fixture, on |p - p_ref| / (p_ref + 1e-6): twice the maximum measured on the MI355X, rounded up to
# one significant digit (docs/LAB_encoder_rollout.md: measured max 2.219e-3 head mean, 9.041e-3 per head, 1.238e-4 the two rollouts).
E2E_BOUND_MEAN = 5e-3
E2E_BOUND_HEAD = 2e-2
E2E_BOUND_ROLLOUT = 3e-4


def self_maps_ref(qkv, B, S, q_rows=None, scale=0.125, rows=None):
    """fp64 restatement -> per-head probabilities (B, 12, S, S), rows q_rows.. zeros.  qkv: (B * S, 2304) bf16 or fp32, one row
    [q | k | v] x [head][64].  rows: only these query rows are computed -> (B, 12, len(rows), S)."""
    q_rows = S if q_rows is None else q_rows
    x = torch.as_tensor(qkv).detach().cpu().to(torch.float64).view(B, S, 3, NH, HD)
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)          # (B, 12, S, 64)
    if rows is not None:
        q = q[:, :, list(rows)]
    s = torch.einsum('bhqd,bhkd->bhqk', q, k)
    c = scale * 1.4426950408889634
    m = torch.ceil(s.max(-1, keepdim=True).values * c)
    p = torch.exp2(s * c - m)
    p = p / p.sum(-1, keepdim=True)
    if rows is None:
        p[:, :, q_rows:] = 0.0
    return p


def make_qkv(B, S, seed, planted=False):
    """bf16 qkv (B * S, 2304), N(0, 1).  planted: in heads 0..3 every query row holds one key that takes nearly all of the row -- key
    (7 * q + 3 * h + b) % S is a copy of 4 q (score 4 |q|^2 * 0.125, about 32, against N(0, 1) for the others; a later query that
    picks the same key overwrites it, so only some rows keep their peak, which is what the test wants: both kinds of row)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, S, 3, NH, HD), generator=g)
    if planted:
        x = x.to(torch.bfloat16).float()
        for b in range(B):
            for h in range(4):
                for q in range(S):
                    x[b, (7 * q + 3 * h + b) % S, 1, h] = 4.0 * x[b, q, 0, h]
    return x.view(B * S, QKV_LD).to(torch.bfloat16)


def op_violations(got, want):
    """Elements that miss |p - p_ref| <= OP_REL * p_ref + OP_ABS -> (count, worst |diff| / bound)."""
    got = torch.as_tensor(got).detach().cpu().to(torch.float64)
    want = torch.as_tensor(want).detach().cpu().to(torch.float64)
    ratio = (got - want).abs() / (OP_REL * want + OP_ABS)
    return int((ratio > 1.0).sum()), float(ratio.max())


def rel_metric(got, want):
    """|p - p_ref| / (p_ref + 1e-6) over the elements -> (max, rms)."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    r = np.abs(got - want) / (want + 1e-6)
    return float(r.max()), float(np.sqrt((r * r).mean()))


def step_ref(v, A, residual):
    """One rollout step in fp64: v (n_img, rows, S), A (n_img, S, S)."""
    v = torch.as_tensor(v).detach().cpu().to(torch.float64)
    A = torch.as_tensor(A).detach().cpu().to(torch.float64)
    return residual * v + (1.0 - residual) * torch.matmul(v, A)


def step_violations(got, want, n_steps=1):
    """Elements that miss |v - v_ref| <= ((1 + gamma)^n - 1) * v_ref + 1e-30 -> (count, worst |diff| / bound)."""
    got = torch.as_tensor(got).detach().cpu().to(torch.float64)
    want = torch.as_tensor(want).detach().cpu().to(torch.float64)
    ratio = (got - want).abs() / (step_rel(n_steps) * want + STEP_ABS)
    return int((ratio > 1.0).sum()), float(ratio.max())


PATH_MUTATIONS = ('caption_path', 'forward', 'swap_adjacent', 'skip_block', 'residual_0')


def rollout_rows_ref(A, w, residual=0.5, mutate=None, step=step_ref):
    """The path of vitcap_amd.rollout.rollout_rows in fp64.  A: (16, n_img, 577, 577) in BLOCK_NAMES order (tag_blocks.3: only its
    row 0 is read); w: (n_img, rows, 578) over [tag-branch cls | cls | 576 patches] -> (n_img, rows, 577).
    mutate: one of PATH_MUTATIONS, a deliberately wrong walk for the comparator's teeth."""
    assert mutate is None or mutate in PATH_MUTATIONS
    A = torch.as_tensor(A).detach().cpu().to(torch.float64)
    w = torch.as_tensor(w).detach().cpu().to(torch.float64)
    r = 0.0 if mutate == 'residual_0' else residual
    cap = [11, 10, 9, 8]
    tag = [14, 13, 12]
    trunk = [7, 6, 5, 4, 3, 2, 1, 0]
    if mutate == 'caption_path':
        tag = [10, 9, 8]
    if mutate == 'forward':
        cap, tag, trunk = cap[::-1], tag[::-1], trunk[::-1]
    if mutate == 'swap_adjacent':
        trunk[2], trunk[3] = trunk[3], trunk[2]
    if mutate == 'skip_block':
        trunk.remove(4)
    v_cap = w[..., 1:]
    for b in cap:
        v_cap = step(v_cap, A[b], r)
    last = A[11 if mutate == 'caption_path' else 15][:, 0, :]                     # (n_img, 577): the last tag block's cls row
    e0 = torch.zeros(NV, dtype=torch.float64)
    e0[0] = 1.0
    v_tag = w[..., 0:1] * (r * e0 + (1.0 - r) * last[:, None, :])
    for b in tag:
        v_tag = step(v_tag, A[b], r)
    v = v_cap + v_tag
    for b in trunk:
        v = step(v, A[b], r)
    return v


def planted_matrices(seed=7, n_img=1, S=NV):
    """16 row-stochastic softmax(12 * randn) matrices per image: sharp rows, so that every block leaves its own mark on the path.
    -> float32 (16, n_img, S, S); the last tag block keeps its cls row only, as the engine writes it."""
    g = torch.Generator().manual_seed(seed)
    A = torch.softmax(12.0 * torch.randn((NB, n_img, S, S), generator=g, dtype=torch.float64), -1).to(torch.float32)
    A[15, :, 1:] = 0.0
    return A


def e0_weights(n_img):
    w = torch.zeros((n_img, 1, NVIS), dtype=torch.float32)
    w[..., 0] = 1.0
    return w


def ecls_weights(n_img):
    w = torch.zeros((n_img, 1, NVIS), dtype=torch.float32)
    w[..., 1] = 1.0
    return w


def random_stochastic(n_img, S, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(3.0 * torch.randn((n_img, S, S), generator=g), -1).to(torch.float32)


def random_rows(n_img, rows, S, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.rand((n_img, rows, S), generator=g)
    return (v / v.sum(-1, keepdim=True)).to(torch.float32)


# ---- the oracle's ViT with its qkv kept (CPU tests): fp32, the reference's arithmetic restated in oracle/vitcap_oracle.py
def oracle_qkv(sd, image):
    """fp32 qkv (B * 577, 2304) of all 16 blocks in BLOCK_NAMES order, from the oracle's ViT on `image` (B, 3, 384, 384)."""
    from oracle import vitcap_oracle as O
    out = [None] * NB

    def block(p, x, slot):
        h = O._ln(sd, p + '.norm1', x, 1e-6)
        out[slot] = O._lin(sd, p + '.attn.qkv', h).reshape(-1, QKV_LD)
        return O.vit_block(sd, p, x)

    with torch.no_grad():
        h = O.patch_embed(sd, image)
        for i in range(FORK):
            h = block('module.bert.encoder.blocks.%d' % i, h, i)
        t = h
        for i in range(FORK, 12):
            h = block('module.bert.encoder.blocks.%d' % i, h, i)
        for i in range(4):
            t = block('module.bert.encoder.tag_blocks.%d' % i, t, 12 + i)
    return out


FIX_ROWS = (0, 289, 576)
FIX_HEAD_BLOCKS = (0, 11, 15)
