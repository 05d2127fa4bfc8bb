"""Test helper of the attention-map tests (tests/test_attn_maps_cpu.py, tests/test_hip_attn_maps.py): an fp64 torch restatement of
the map row that vitcap_attn_probe_maps defines (include/vitcap_hip.h), the inputs both suites feed it, and the two comparators with
their bounds.  Pure torch / numpy on the CPU; nothing here touches the GPU library.

The row: caption c, position t = 1..L-1, head h.  The [MASK] probe at grid row L + t - 1 attends the image's 578 visual rows, token
rows 0..t-1 and itself; width W = 578 + L, columns [578 visual | token k at 578 + k, k < t | the probe at 578 + t | zeros].  Softmax in
the log2 domain, m = ceil(max * c), p = exp2(s * c - m), row = p / sum(p).  Position 0 and positions behind the caption's first end
token are zeros."""
import math

import numpy as np
import torch

NVIS, NH, HD, QKV_LD = 578, 12, 64, 2304
EOS = 102

# |p - p_ref| <= OP_REL * p_ref + OP_ABS: fp32 accumulation of a 64-term bf16 dot product costs at most 64 * 2^-24 * sum|q_i k_i|
# (about 3e-4 on N(0,1) inputs), times the 0.125 scale, plus a row sum of about 620 fp32 terms.  Derived, not measured.
OP_REL, OP_ABS = 2e-4, 1e-7
# End to end against the reference fixture, on |p - p_ref| / (p_ref + 1e-6): twice the maximum measured on the MI355X, rounded up to
# one significant digit (docs/LAB_attention_maps.md: measured max 2.24e-3 head mean, 8.69e-3 per head).
E2E_BOUND_MEAN = 5e-3
E2E_BOUND_HEAD = 2e-2

MUTATIONS = ('sees_token_t', 'no_self', 'vis_shift', 'head_swap')


def live_rows(caption_ids, eos=EOS, eos_extra=()):
    """(n_caps, L) int64 -> bool (n_caps, L): position t >= 1 holds a decision while no end token stands at a position 1..t-1."""
    ids = torch.as_tensor(caption_ids)
    is_eos = ids == eos
    for e in eos_extra:
        is_eos = is_eos | (ids == int(e))
    is_eos[:, 0] = False
    ended_before = torch.cumsum(is_eos.to(torch.int64), 1) - is_eos.to(torch.int64) > 0
    live = ~ended_before
    live[:, 0] = False
    return live


def probe_maps_ref(qkv_text, vis_qkv, caption_ids, n_images, caps_per_image, max_len, eos=EOS, eos_extra=(), scale=0.125,
                   mutate=None):
    """fp64 restatement -> per-head maps, float64 (n_caps, L, 12, W).  qkv_text bf16 (n_caps * (2L - 1), 2304), vis_qkv bf16
    (n_images * 578, 2304).  mutate: one of MUTATIONS, a deliberately wrong variant for the comparator's teeth."""
    assert mutate is None or mutate in MUTATIONS
    L, R, NC, W = max_len, 2 * max_len - 1, n_images * caps_per_image, NVIS + max_len
    x = qkv_text.detach().cpu().to(torch.float64).view(NC, R, QKV_LD)
    v = vis_qkv.detach().cpu().to(torch.float64).view(n_images, NVIS, QKV_LD)
    q = x[:, L:, :768].reshape(NC, L - 1, NH, HD)                    # probe j = t - 1
    k_tok = x[:, :L, 768:1536].reshape(NC, L, NH, HD)
    k_self = x[:, L:, 768:1536].reshape(NC, L - 1, NH, HD)
    k_vis = v[:, :, 768:1536].reshape(n_images, NVIS, NH, HD).repeat_interleave(caps_per_image, 0)
    s = torch.full((NC, L - 1, NH, W), -math.inf, dtype=torch.float64)
    s_vis = torch.einsum('cjhd,ckhd->cjhk', q, k_vis)
    if mutate == 'vis_shift':
        s_vis = torch.roll(s_vis, 1, -1)
    s[..., :NVIS] = s_vis
    s_tok = torch.einsum('cjhd,ckhd->cjhk', q, k_tok)                # (NC, L-1, NH, L)
    j = torch.arange(L - 1).view(1, L - 1, 1, 1)
    kk = torch.arange(L).view(1, 1, 1, L)
    seen = kk <= (j + 1 if mutate == 'sees_token_t' else j)          # token keys 0..t-1 = 0..j
    s[..., NVIS:] = torch.where(seen, s_tok, torch.full_like(s_tok, -math.inf))
    if mutate != 'no_self':
        s_self = (q * k_self).sum(-1)                                # (NC, L-1, NH)
        idx = (NVIS + 1 + torch.arange(L - 1)).view(1, L - 1, 1, 1).expand(NC, L - 1, NH, 1)
        if mutate == 'sees_token_t':                                 # token t's mass lands in the probe's column
            s_self = torch.logaddexp(s_self * scale, s.gather(-1, idx).squeeze(-1) * scale) / scale      # both share column 578 + t
        s.scatter_(-1, idx, s_self.unsqueeze(-1))
    c = scale * 1.4426950408889634
    m = torch.ceil(s.max(-1, keepdim=True).values * c)
    p = torch.exp2(s * c - m)
    p = p / p.sum(-1, keepdim=True)
    if mutate == 'head_swap':
        p = p.flip(2)
    out = torch.zeros((NC, L, NH, W), dtype=torch.float64)
    out[:, 1:] = p
    out[~live_rows(caption_ids, eos, eos_extra)] = 0.0
    return out


def head_mean(per_head):
    return per_head.mean(-2)


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


def captions(n_caps, max_len, seed):
    """Caption ids (n_caps, L) int64 for the op tests: end tokens at position 1, mid-caption and the last column, plus captions
    with no end token, in turn."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 30000, (n_caps, max_len), generator=g, dtype=torch.int64)
    ids[:, 0] = 101
    for c in range(n_caps):
        kind = c % 4
        end = {0: 1, 1: max(1, max_len // 2), 2: max_len - 1, 3: None}[kind]
        if end is not None:
            ids[c, end] = EOS
            ids[c, end + 1:] = 0
    return ids


def make_inputs(n_images, caps_per_image, max_len, seed, planted=False):
    """bf16 qkv_text (n_caps * (2L - 1), 2304) and vis_qkv (n_images * 578, 2304), N(0, 1).  planted: per probe one key whose score
    dominates its row by a known gap -- the key is a copy of the probe's own q (score |q|^2 * 0.125, about 8, against N(0, 1) for
    every other key): in head 0 the TOKEN key at the probe's own position t (which the probe must not see), in head 1 the probe's
    own key, in head 2 visual key (37 * t + 5 * c) % 578, in head 3 token key t - 1 (the last one it does see)."""
    L, R, NC = max_len, 2 * max_len - 1, n_images * caps_per_image
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((NC, R, QKV_LD), generator=g)
    v = torch.randn((n_images, NVIS, QKV_LD), generator=g)
    if planted:
        x = x.to(torch.bfloat16).float()
        for c in range(NC):
            for t in range(1, L):
                qrow = x[c, L + t - 1, :768].view(NH, HD)
                x[c, t, 768 + 0 * HD:768 + 1 * HD] = qrow[0]
                x[c, L + t - 1, 768 + 1 * HD:768 + 2 * HD] = qrow[1]
                x[c, t - 1, 768 + 3 * HD:768 + 4 * HD] = qrow[3]
        for c in range(NC):
            for t in range(1, L, 3):      # a third of the probes: visual keys are shared by the image's captions
                v[c // caps_per_image, (37 * t + 5 * c) % NVIS, 768 + 2 * HD:768 + 3 * HD] = x[c, L + t - 1, 2 * HD:3 * HD]
    return x.view(NC * R, QKV_LD).to(torch.bfloat16), v.view(n_images * NVIS, QKV_LD).to(torch.bfloat16)
