"""Test helper of the region-captions-under-beam-search tests (tests/test_region_beam_cpu.py, tests/test_hip_region_beams.py): what
vitcap_attn_decode_beam_groups_masked defines (include/vitcap_hip.h) restated through region_ref.decode_ref, the mask kinds that sit
on this kernel's edges, planted inputs, deliberately wrong variants for the comparator's teeth, the comparator itself, and the
end-to-end reference: the reference's beam driver (oracle.beam_bookkeeping) around the as-written forward with the visual columns
hidden from the caption rows.  Pure torch on the CPU; region_ref and occlusion_ref are used as they are.

The op: group g = sequences [g K, (g + 1) K) of the batch, image g // groups_per_image; ONE mask row per group, obeyed by both query
rows of all K sequences; the text keys never consult it."""
import math

import torch

import occlusion_ref as OR
import region_ref as RR

NH, HD = RR.NH, RR.HD
MUTATIONS = ('bit_shift', 'wrong_group', 'text_masked', 'even_rows_only')

# region_ref's kinds (random, all_hidden, only_0, only_last, hide_128_255, only_0_127, bit_31 / 32 -- the word and 32-key block edge --,
# bit_127 / 128, bit_last) and the edges of THIS kernel: bit 15 / 16 the 16-key block edge, bit 63 / 64 the four waves' block stride,
# only_16_31 a live half of a live word (its other half is skipped in phase 1a and must still read as -inf in phase 2a), hide_32_63 a
# zero word between live ones (skipped in both phases)
MASK_KINDS = RR.MASK_KINDS + ('bit_15', 'bit_16', 'bit_63', 'bit_64', 'only_16_31', 'hide_32_63')


def kinds_for(S):
    base = RR.kinds_for(S)
    return tuple(k for k in MASK_KINDS if (k in base if k in RR.MASK_KINDS else
                                           (S > 33 if k in ('only_16_31', 'hide_32_63') else int(k[4:]) < S - 1)))


def mask_of_kind(kind, S, gen):
    """bool (S,), True = visible."""
    if kind == 'only_16_31':
        m = torch.zeros(S, dtype=torch.bool)
        m[16:32] = True
        return m
    if kind == 'hide_32_63':
        m = torch.ones(S, dtype=torch.bool)
        m[32:64] = False
        return m
    return RR.mask_of_kind(kind, S, gen)


def masks_by_kind(G, S, seed, first=0):
    """bool (G, S): group g takes kind (first + g) % len(kinds_for(S)); the random ones differ per group."""
    gen = torch.Generator().manual_seed(seed)
    kinds = kinds_for(S)
    return torch.stack([mask_of_kind(kinds[(first + g) % len(kinds)], S, gen) for g in range(G)])


pack_bits = RR.pack_bits        # (G, S) bool -> int32 (G, words); high_bits = True sets the bits from S on, which the kernel ignores


def decode_ref(vis, cache, step, t, K, gpi, group_mask=None, emulate=True):
    """-> (B, 2, 768), B = n_images * gpi * K.  group_mask bool (n_images * gpi, S) or None: every sequence of a group obeys its row."""
    v = None if group_mask is None else torch.as_tensor(group_mask).bool().repeat_interleave(K, 0)
    return RR.decode_ref(vis, cache, step, t, K * gpi, visible=v, emulate=emulate)


def decode_mutant(vis, cache, step, t, K, gpi, group_mask, mutate, emulate=False):
    """The same mathematics with one deliberate mistake (None: none, equal to decode_ref):
      bit_shift       key k reads bit k + 1;
      wrong_group     group g reads group g - 1's row (group 0 the last one's); with several groups per image, its image's row g // gpi
                      (a kernel that indexes the mask by image);
      text_masked     text key j also obeys bit j;
      even_rows_only  only row 0 of each sequence (the even query rows of the group) obeys the mask, the [MASK] rows see everything."""
    assert mutate is None or mutate in MUTATIONS
    dt = torch.float32 if emulate else torch.float64
    gm = torch.as_tensor(group_mask).bool().clone()
    G, S = gm.shape
    B = step.shape[0]
    assert B == G * K and vis.shape[0] * gpi == G
    if mutate == 'bit_shift':
        gm = torch.cat([gm[:, 1:], torch.zeros(G, 1, dtype=torch.bool)], 1)
    if mutate == 'wrong_group':
        gm = torch.roll(gm, 1, 0) if gpi == 1 else gm[torch.arange(G) // gpi]
    seq = gm.repeat_interleave(K, 0)
    allow = torch.ones(B, 2, S + t + 1, dtype=torch.bool)
    allow[:, :, :S] = seq[:, None, :]
    if mutate == 'even_rows_only':
        allow[:, 1, :S] = True
    if mutate == 'text_masked':
        n = min(t, S)
        allow[:, :, S:S + n] &= seq[:, None, :n]
    allow[:, 0, -1] = False                      # row 0 (position t-1) does not see the [MASK] row
    visr = vis.repeat_interleave(K * gpi, 0).to(dt)
    Kk = torch.cat([visr[..., 768:1536], cache[:, :t - 1, 0].to(dt), step[:, :, 768:1536].to(dt)], 1)
    V = torch.cat([visr[..., 1536:], cache[:, :t - 1, 1].to(dt), step[:, :, 1536:].to(dt)], 1)
    q = step[..., :768].to(dt).view(B, 2, NH, HD).transpose(1, 2)
    s = q @ Kk.view(B, -1, NH, HD).transpose(1, 2).transpose(-1, -2)
    s = s.masked_fill(~allow[:, None], -math.inf)
    Vh = V.view(B, -1, NH, HD).transpose(1, 2)
    if emulate:
        from oracle import vitcap_oracle as O
        o = O.softmax_pv_rounded(s, Vh, O._R(True))
    else:
        m = torch.ceil(s.max(-1, keepdim=True).values * RR.C_LOG2)
        p = torch.exp2(s * RR.C_LOG2 - m)
        o = (p @ Vh) / p.sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(B, 2, 768)


# ---- the comparator of tests/test_hip_region_beams.py test 1.  The bound is what vitcap_attn_decode_beam_groups (the plain entry
# point, whose two instances are instruction for instruction the parent commit's) meets against decode_ref with everything visible
# on the random and planted inputs of shapes() below, stated as a + r |want|: with r fixed by the number formats, the largest
# |err| - r |want| over all 46 input sets was 2.933e-4 (S_vis = 47, K = 8, t = 19, three groups per image; tests/
# test_hip_region_beams.py::plain_bound, docs/LAB_region_beams.md section 2).  The masked rows hold fewer, larger probabilities, so
# the test allows twice that.
BOUND_R = 2.0 ** -8          # half a bf16 ulp of the output (2^-9) and as much again for the bf16 rounding of P
MEASURED_A = 2.933e-4        # the observed maximum, not rounded up
BOUND_MARGIN = 2.0


def bound(want):
    return BOUND_MARGIN * (MEASURED_A + BOUND_R * torch.as_tensor(want).detach().double().cpu().abs())


def excess(got, want):
    """-> (elements that miss bound(want), max |err|, max of |err| - BOUND_R |want|: the `a` the pair would need at margin 1)."""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    err = (got - want).abs()
    return int((err > bound(want)).sum()), float(err.max()), float((err - BOUND_R * want.abs()).max())


# ---- shapes and inputs
S_VIS = (47, 578, 608)        # three 16-key blocks, the last short, one word edge | the model's | no padding keys
KTL = ((2, 1, 20), (5, 19, 20), (8, 19, 20), (3, 40, 41))      # (K, t, max_len): the first two run the <4, 3> instance
GPI = (1, 3)
N_IMAGES = 2


def shapes():
    return [(S, K, t, ml, gpi) for S in S_VIS for (K, t, ml) in KTL for gpi in GPI]


def random_inputs(S, K, t, max_len, gpi, n_images=N_IMAGES):
    """(vis (n_images, S, 2304), cache (B, max_len, 2, 768), step (B, 2, 2304)) bf16, U(-2, 2); B = n_images * gpi * K."""
    B = n_images * gpi * K
    bf = torch.bfloat16
    return (RR._rand((n_images, S, 2304), 900 + S, 2.0).to(bf), RR._rand((B, max_len, 2, 768), 901 + S + B, 2.0).to(bf),
            RR._rand((B, 2, 2304), 910 + t + B, 2.0).to(bf))


def can_plant(S, K, gpi, n_images=N_IMAGES):
    return (S - 1) // (2 * n_images * gpi * K) >= 1


def planted_inputs(S, K, t, max_len, gpi, n_images=N_IMAGES):
    """random_inputs reworked in the manner of region_ref.planted_inputs: per (sequence b, query row r, head h < nh) one visual key of
    the sequence's image is TWICE that row's q in head h and zero in every other head, and is hidden from the sequence; text key 0 is
    twice the PROBE row's q in head TEXT_HEAD, visual key 0 is zero and hidden everywhere.  A GROUP's mask is the AND of its
    sequences' masks: it hides the planted keys of all K of them (a sibling's planted key is an ordinary key to the others).
    nh = min(12, (S - 1) // (2 B)).  -> (vis, cache, step, group_mask bool (n_images * gpi, S))."""
    vis, cache, step = (x.clone() for x in random_inputs(S, K, t, max_len, gpi, n_images))
    B, spi = step.shape[0], K * gpi
    nh = min(NH, (S - 1) // (2 * B))
    assert nh >= 1
    keys = {(b, r, h): RR.planted_key(b, r, h, nh, S) for b in range(B) for r in range(2) for h in range(nh)}
    assert len(set(keys.values())) == len(keys) and 0 not in keys.values()
    visible = torch.ones(B, S, dtype=torch.bool)
    vis[:, 0, 768:1536] = 0
    visible[:, 0] = False
    for (b, r, h), k in keys.items():
        vis[b // spi, k, 768:1536] = 0
        vis[b // spi, k, 768 + h * HD:768 + (h + 1) * HD] = (2 * step[b, r, h * HD:(h + 1) * HD].float()).to(torch.bfloat16)
        visible[b, k] = False
    th = RR.TEXT_HEAD
    for b in range(B):
        twice = (2 * step[b, 1, th * HD:(th + 1) * HD].float()).to(torch.bfloat16)
        if t == 1:
            step[b, 0, 768 + th * HD:768 + (th + 1) * HD] = twice
        else:
            cache[b, 0, 0, th * HD:(th + 1) * HD] = twice
    return vis, cache, step, visible.view(B // K, K, S).all(1)


# ---- end to end: the reference's beam search with visual columns hidden from the caption rows
def masked_stepper(sd, image, K, visible, max_length, enc=None):
    """oracle._as_written_stepper with the masked joint mask of region_ref.greedy_as_written_masked: the visual columns where
    `visible` (B, 578) is False are zeroed in the caption rows, key 577 through joint_forward_masked's last_col.  All K beams of an
    image obey its row.  -> step(input_ids (B*K, cur_len), beam_idx) -> next-token logits (B*K, V)."""
    from oracle import vitcap_oracle as O
    NVIS = OR.NVIS
    B = image.shape[0]
    img_feats = O.patch_embed(sd, image)
    if enc is None:
        enc = O.split_encoder(sd, img_feats)
    input_ids0, am = O.test_text_inputs(B, max_length)
    full_mask = O.construct_attn_mask(am, img_feats.shape[1])
    rep = lambda x: x.repeat_interleave(K, 0)
    full_mask_k, enc_k, od = rep(full_mask), (rep(enc[0]), rep(enc[1])), rep(input_ids0[:, max_length:])
    vis_k = rep(torch.as_tensor(visible).bool())
    pos_full = torch.cat([torch.arange(max_length), torch.arange(20, 20 + O.OD_LEN)])

    def step(input_ids, beam_idx):
        cur = input_ids.shape[1]
        curr = cur + 1
        ids = torch.cat([input_ids, torch.full((B * K, 1), O.MASK, dtype=torch.long), od], dim=1)
        mask = O._remove_rows_cols(full_mask_k, curr, max_length, curr, max_length).clone()
        T = curr + O.OD_LEN
        mask[:, :curr, T:] *= vis_k[:, None, :NVIS - 1].to(mask.dtype)
        last_col = torch.ones(B * K, mask.shape[1] + 1)
        last_col[:, :curr] = vis_k[:, NVIS - 1:].to(mask.dtype)
        pp = torch.cat([pos_full[:curr], pos_full[max_length:]]).unsqueeze(0).expand(B * K, -1)
        tt = torch.zeros(B * K, curr + O.OD_LEN, dtype=torch.long)
        seq = OR.joint_forward_masked(sd, ids, mask, last_col, pp, tt, enc_k)
        return O.lm_head(sd, 'module.cls', seq[:, cur:cur + 1])[:, 0]
    return step, enc


def beam_masked(sd, image, visible, K, max_length, num_keep_best=1, length_penalty=1.0, enc=None):
    """-> (ids (B, keep, L), scores (B, keep), margins (B, L - 1), enc)."""
    from oracle import vitcap_oracle as O
    step, enc = masked_stepper(sd, image, K, visible, max_length, enc)
    ids, lp, mg = O.beam_bookkeeping(step, image.shape[0], K, max_length, length_penalty=length_penalty, num_keep_best=num_keep_best,
                                     return_margins=True)
    return ids, lp, mg, enc


# ---- the end-to-end case of tests/test_hip_region_beams.py test 5: region_ref's images and masks, CASE_K beams, the two best kept
CASE_L, CASE_K, CASE_KEEP = RR.CASE_L, 3, 2
CASE_FILE = 'region_beam_captions.npz'       # under tests/golden: the reference's results, so that the GPU test computes none
CASE_MASKS = ('unmasked', 'box', 'nothing')


def case_inputs():
    """-> (images (2, 3, 384, 384), visible bool (2, 3, 578)): per image everything, its box of region_ref.CASE_BOXES with the cls
    columns, and nothing."""
    img, vis = RR.case_inputs()
    return img, torch.cat([torch.ones(2, 1, OR.NVIS, dtype=torch.bool), vis], 1)


def build_case(sd, images=(0, 1), masks=(0, 1, 2)):
    """The reference's results as numpy arrays, per mask of CASE_MASKS: ids (2, 3, keep, L), scores (2, 3, keep), margins
    (2, 3, L - 1).  `images` / `masks`: the subset to compute (the rest stays zero)."""
    img, vis = case_inputs()
    L = CASE_L
    ids = torch.zeros(2, 3, CASE_KEEP, L, dtype=torch.long)
    scores, margins = torch.zeros(2, 3, CASE_KEEP), torch.zeros(2, 3, L - 1)
    sel = list(images)
    enc = None
    with torch.no_grad():
        for j in masks:
            i_, s_, m_, enc = beam_masked(sd, img[sel], vis[sel, j], CASE_K, L, num_keep_best=CASE_KEEP, enc=enc)
            ids[sel, j], scores[sel, j], margins[sel, j] = i_, s_, m_
    return {'ids': ids.numpy(), 'scores': scores.numpy(), 'margins': margins.numpy()}


if __name__ == '__main__':      # python tests/beam_masked_ref.py: writes tests/golden/region_beam_captions.npz
    import os
    import sys

    import numpy as np
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    from oracle import vitcap_oracle as O
    from vitcap_amd import weights as W
    case = build_case(O.to_torch(W.make_state_dict(seed=0, tie_weights=True)))
    np.savez(os.path.join(here, 'golden', CASE_FILE), **case)
    for k, v in case.items():
        print(k, v.tolist())
