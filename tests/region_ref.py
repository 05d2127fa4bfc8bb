"""Test helper of the region-caption tests (tests/test_region_cpu.py, tests/test_hip_regions.py): a torch restatement of the masked
decode-step attention that vitcap_attn_decode_step_masked defines (include/vitcap_hip.h) -- the rounding-emulated fp32 reference of
tests/test_hip_attn_decode_kv.py::_reference with a `visible` argument, and the same mathematics in fp64 --, the masks and planted
inputs both suites feed it, deliberately wrong variants for the comparator's teeth, and the end-to-end reference: the loop of
occlusion_ref.token_logprobs_as_written with argmax in place of the given token.  Pure torch on the CPU.

The op: sequence b of image b // spi, two query rows (row 0 the token at position t-1, row 1 the [MASK] probe).  Keys: the image's
S visual rows, visible to BOTH rows where bit k of the sequence's mask is set, then the cached text rows 0..t-2, this step's row 0
and, for row 1 only, this step's row 1 -- none of which the mask touches."""
import math

import torch

import occlusion_ref as OR

NH, HD, QKV_LD = 12, 64, 2304
C_LOG2 = OR.C_LOG2
LCACHE = 20               # text cache rows per sequence

MUTATIONS = ('bit_shift', 'wrong_sequence', 'probe_row_only', 'text_masked')

# the kinds of test 1 of tests/test_hip_regions.py; a kind that needs more keys than S has is left out at that S (kinds_for)
MASK_KINDS = ('random', 'all_hidden', 'only_0', 'only_last', 'hide_128_255', 'only_0_127', 'bit_31', 'bit_32', 'bit_127', 'bit_128',
              'bit_last')


def kinds_for(S):
    return tuple(k for k in MASK_KINDS
                 if not ((k == 'hide_128_255' and S < 256) or (k == 'only_0_127' and S <= 128)
                         or (k.startswith('bit_') and k != 'bit_last' and int(k[4:]) >= S - 1)))


def mask_of_kind(kind, S, gen):
    """bool (S,), True = visible."""
    if kind == 'random':
        return torch.rand(S, generator=gen) < 0.5
    m = torch.ones(S, dtype=torch.bool)
    if kind == 'all_hidden':
        m[:] = False
    elif kind == 'only_0':
        m[:] = False
        m[0] = True
    elif kind == 'only_last':
        m[:] = False
        m[S - 1] = True
    elif kind == 'hide_128_255':
        m[128:256] = False
    elif kind == 'only_0_127':
        m[128:] = False
    elif kind == 'bit_last':
        m[S - 1] = False
    else:
        m[int(kind[4:])] = False
    return m


def masks_by_kind(B, S, seed, first=0):
    """bool (B, S): sequence i takes kind (first + i) % len(kinds_for(S)); the random ones differ per sequence."""
    g = torch.Generator().manual_seed(seed)
    kinds = kinds_for(S)
    return torch.stack([mask_of_kind(kinds[(first + i) % len(kinds)], S, g) for i in range(B)])


def pack_bits(visible, words=None, high_bits=False):
    """bool (B, S) -> int32 (B, words >= ceil(S / 32)): bit k & 31 of word k >> 5 is key k; the bits from S on are clear, or with
    high_bits all set (the kernel must ignore them)."""
    v = torch.as_tensor(visible).bool()
    B, S = v.shape
    words = words or (S + 31) // 32
    bits = torch.full((B, words * 32), 1 if high_bits else 0, dtype=torch.int64)
    bits[:, :S] = v.to(torch.int64)
    w = (bits.view(B, words, 32) << torch.arange(32, dtype=torch.int64)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def _allow(visible, B, S, t, mutate):
    """(B, 2, S + t + 1) bool: what query row r of sequence b may attend, with the mutation applied."""
    assert mutate is None or mutate in MUTATIONS
    vis = torch.as_tensor(visible).bool().clone()
    assert tuple(vis.shape) == (B, S)
    if mutate == 'bit_shift':                    # key k reads bit k + 1 (the bit behind the last key is a clear padding bit)
        vis = torch.cat([vis[:, 1:], torch.zeros(B, 1, dtype=torch.bool)], 1)
    if mutate == 'wrong_sequence':               # sequence b reads sequence b - 1's mask (sequence 0 the last one's)
        vis = torch.roll(vis, 1, 0)
    allow = torch.ones(B, 2, S + t + 1, dtype=torch.bool)
    allow[:, :, :S] = vis[:, None, :]
    if mutate == 'probe_row_only':               # row 0 sees every visual key
        allow[:, 0, :S] = True
    if mutate == 'text_masked':                  # text key j also obeys bit j
        n = min(t, S)
        allow[:, :, S:S + n] &= vis[:, None, :n]
    allow[:, 0, -1] = False                      # row 0 (position t-1) does not see the [MASK] row
    return allow


def decode_ref(vis, cache, step, t, spi, visible=None, mutate=None, emulate=True):
    """-> (B, 2, 768).  vis bf16 (B // spi, S, 2304) visual q|k|v rows per image, cache bf16 (B, LCACHE, 2, 768), step bf16 (B, 2, 2304),
    visible bool (B, S) or None (everything visible).  emulate: the device's rounding points (oracle.softmax_pv_rounded: fp32 scores,
    m = ceil(max * c), bf16 P for the product, the row sum from the unrounded P), fp32; otherwise the same mathematics in float64."""
    dt = torch.float32 if emulate else torch.float64
    B, S = step.shape[0], vis.shape[1]
    if visible is None:
        visible = torch.ones(B, S, dtype=torch.bool)
    visr = vis.repeat_interleave(spi, 0).to(dt)
    K = torch.cat([visr[..., 768:1536], cache[:, :t - 1, 0].to(dt), step[:, :, 768:1536].to(dt)], 1)
    V = torch.cat([visr[..., 1536:], cache[:, :t - 1, 1].to(dt), step[:, :, 1536:].to(dt)], 1)
    q = step[..., :768].to(dt).view(B, 2, NH, HD).transpose(1, 2)
    s = q @ K.view(B, -1, NH, HD).transpose(1, 2).transpose(-1, -2)              # (B, 12, 2, S + t + 1)
    s = s.masked_fill(~_allow(visible, B, S, t, mutate)[:, None], -math.inf)
    Vh = V.view(B, -1, NH, HD).transpose(1, 2)
    if emulate:
        from oracle import vitcap_oracle as O
        o = O.softmax_pv_rounded(s, Vh, O._R(True))
    else:
        m = torch.ceil(s.max(-1, keepdim=True).values * C_LOG2)
        p = torch.exp2(s * C_LOG2 - m)
        o = (p @ Vh) / p.sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(B, 2, 768)


violations = OR.violations        # elements that miss |err| <= 2e-3 + 2^-7 |want| -> (count, max |err|)


# ---- random and planted inputs
def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def n_seq(spi):
    """3 sequences; with two sequences per image the entry point wants whole images, so 4 (two images)."""
    return 3 if spi == 1 else 4


def random_inputs(S, spi, t, B=None):
    """(vis (B // spi, S, 2304), cache (B, LCACHE, 2, 768), step (B, 2, 2304)) bf16, U(-2, 2) like tests/test_hip_attn_decode_kv.py."""
    B = B or n_seq(spi)
    bf = torch.bfloat16
    return (_rand((B // spi, S, 2304), 700 + S, 2.0).to(bf), _rand((B, LCACHE, 2, 768), 701 + S, 2.0).to(bf),
            _rand((B, 2, 2304), 710 + t, 2.0).to(bf))


PLANT_STRIDE, PLANT_FIRST = 5, 7
TEXT_HEAD = 0             # the head in which text key 0 dominates the probe row (for 'text_masked')


def planted_key(b, r, h, nh, S):
    return 1 + (PLANT_FIRST + PLANT_STRIDE * (b * 2 * nh + r * nh + h)) % (S - 1)      # never key 0


def planted_inputs(S, spi, t):
    """random_inputs reworked so that hiding keys visibly moves rows:
      * per (sequence b, query row r, head h < nh) one visual key of the sequence's image is TWICE that row's q in head h and zero in
        every other head -- it scores 2 |q|^2 / 8, about 21 against a deviation of 1.3 for the other keys, and holds the row -- and
        sequence b's mask hides exactly its own 2 nh planted keys; nh = min(12, (S - 1) // (2 B)) so that all B * 2 * nh keys are distinct;
      * text key 0 (cache row 0, or at t = 1 this step's row 0) is twice the PROBE row's q in head TEXT_HEAD, visual key 0 is zero
        in every head and hidden in every mask: with the right semantics the text key then holds (probe, TEXT_HEAD); a kernel that
        lets text key j obey bit j loses it.
    The planted keys of one sequence are never neighbours, so a mask read one bit off shows them.
    -> (vis, cache, step, visible bool (B, S))."""
    vis, cache, step = (x.clone() for x in random_inputs(S, spi, t))
    B = step.shape[0]
    nh = min(NH, (S - 1) // (2 * B))
    assert nh >= 1
    keys = {}
    for b in range(B):
        for r in range(2):
            for h in range(nh):
                keys[(b, r, h)] = planted_key(b, r, h, nh, S)
    assert len(set(keys.values())) == len(keys) and 0 not in keys.values()
    visible = torch.ones(B, S, dtype=torch.bool)
    vis[:, 0, 768:1536] = 0
    visible[:, 0] = False
    for (b, r, h), k in keys.items():
        mine = set(keys[(b, rr, hh)] for rr in range(2) for hh in range(nh))
        assert k + 1 not in mine
        vis[b // spi, k, 768:1536] = 0
        vis[b // spi, k, 768 + h * HD:768 + (h + 1) * HD] = (2 * step[b, r, h * HD:(h + 1) * HD].float()).to(torch.bfloat16)
        visible[b, k] = False
    for b in range(B):
        twice = (2 * step[b, 1, TEXT_HEAD * HD:(TEXT_HEAD + 1) * HD].float()).to(torch.bfloat16)
        if t == 1:
            step[b, 0, 768 + TEXT_HEAD * HD:768 + (TEXT_HEAD + 1) * HD] = twice
        else:
            cache[b, 0, 0, TEXT_HEAD * HD:(TEXT_HEAD + 1) * HD] = twice
    return vis, cache, step, visible


# ---- end to end: greedy decoding with the oracle's forward as written, visual columns hidden from the caption rows
def greedy_as_written_masked(sd, image, visible, max_length, enc=None):
    """The loop of occlusion_ref.token_logprobs_as_written with argmax in place of the given token: one full forward per position
    on [tokens so far, MASK, tag slots] with the visual columns where `visible` (B, 578) is False zeroed in the caption rows of the
    joint mask, the bookkeeping of oracle.greedy_as_written (pad behind the end, the last column forced to [SEP]).
    -> (ids (B, L), logprob (B,), margins (B, L - 1): top-1 minus top-2 logit of every step a sequence was still open at (inf behind
    its end), last (B,): the token chosen at the last position, which the ids overwrite with [SEP], enc)."""
    import torch.nn.functional as F
    from oracle import vitcap_oracle as O
    NVIS = OR.NVIS
    B = image.shape[0]
    visible = torch.as_tensor(visible).bool()
    img_feats = O.patch_embed(sd, image)
    input_ids0, am = O.test_text_inputs(B, max_length)
    full_mask = O.construct_attn_mask(am, img_feats.shape[1])
    od_label_ids = input_ids0[:, max_length:]
    od_len = od_label_ids.shape[1]
    full_pos = torch.arange(max_length + od_len).unsqueeze(0).expand(B, -1)
    full_tt = torch.zeros(B, max_length + od_len, dtype=torch.long)
    if enc is None:
        enc = O.split_encoder(sd, img_feats)
    ids = torch.full((B, 1), O.BOS, dtype=torch.long)
    unfinished = torch.ones(B, dtype=torch.long)
    sum_lp, cnt = torch.zeros(B), torch.zeros(B)
    margins = torch.full((B, max_length - 1), float('inf'))
    for cur_len in range(1, max_length):
        step_ids = torch.cat([ids, torch.full((B, 1), O.MASK, dtype=torch.long)], dim=1)
        curr = step_ids.shape[1]
        mask = O._remove_rows_cols(full_mask, curr, max_length, curr, max_length).clone()
        T = curr + od_len
        mask[:, :curr, T:] *= visible[:, None, :NVIS - 1].to(mask.dtype)
        last_col = torch.ones(B, mask.shape[1] + 1)
        last_col[:, :curr] = visible[:, NVIS - 1:].to(mask.dtype)
        tt = torch.cat([full_tt[:, :curr], full_tt[:, max_length:]], dim=1)
        pp = torch.cat([full_pos[:, :curr], full_pos[:, max_length:]], dim=1)
        seq = OR.joint_forward_masked(sd, torch.cat([step_ids, od_label_ids], dim=1), mask, last_col, pp, tt, enc)
        logits = O.lm_head(sd, 'module.cls', seq[:, cur_len:cur_len + 1])[:, 0]
        top2 = logits.topk(2, dim=-1)
        nxt = top2.indices[:, 0]
        live = unfinished.bool()
        margins[live, cur_len - 1] = (top2.values[:, 0] - top2.values[:, 1])[live]
        lp = torch.gather(F.log_softmax(logits, dim=-1), -1, nxt.unsqueeze(-1)).squeeze(-1)
        sum_lp += lp * unfinished
        cnt += unfinished
        add = nxt * unfinished + O.PAD * (1 - unfinished)
        ids = torch.cat([ids, add.unsqueeze(-1)], dim=-1)
        unfinished = unfinished * add.ne(O.EOS).long()
    ids[:, -1].masked_fill_(unfinished.bool(), O.EOS)
    return ids, sum_lp / cnt, margins, nxt, enc


# ---- the end-to-end case of tests/test_hip_regions.py test 3, chosen in the reference alone (tests/test_region_cpu.py holds the check)
CASE_L, CASE_SEED = 8, 1234          # the images and max_length of tests/test_hip_occlusion.py's end-to-end test, two of them
CASE_BOXES = ((9, 9, 15, 15), (0, 0, 6, 6))      # image 0: the central 6 x 6 patches, image 1: the top-left 6 x 6; cls kept
CASE_FILE = 'region_captions.npz'    # under tests/golden: the reference's results for the case, so that the GPU test computes none


def case_inputs():
    """-> (images (2, 3, 384, 384), visible bool (2, 2, 578)): per image its box of CASE_BOXES with the cls columns, and nothing."""
    from vitcap_amd import regions as RG
    from vitcap_amd import weights as W
    img = torch.from_numpy(W.gen_image_batch(2, CASE_SEED))
    vis = torch.zeros(2, 2, OR.NVIS, dtype=torch.bool)
    vis[:, 0] = RG.box_masks(torch.tensor(CASE_BOXES))
    return img, vis


def build_case(sd):
    """The reference's own results for the case, as numpy arrays: unmasked greedy ids (2, L); per image and mask the greedy ids
    (2, 2, L), margins (2, 2, L - 1), last choice (2, 2), sequence log-prob (2, 2); and token_logprobs_as_written of those captions
    (the last column scored on the last choice where the caption had not ended): tok_lp (2, 2, L), seq_lp (2, 2)."""
    img, vis = case_inputs()
    L = CASE_L
    with torch.no_grad():
        ids_u, _, mg_u, _, enc = greedy_as_written_masked(sd, img, torch.ones(2, OR.NVIS, dtype=torch.bool), L)
        out = {'unmasked_ids': ids_u, 'unmasked_margins': mg_u}
        cols = {k: [] for k in ('ids', 'margins', 'last', 'greedy_lp', 'tok_lp', 'seq_lp')}
        for j in range(2):
            ids, lp, mg, last, _ = greedy_as_written_masked(sd, img, vis[:, j], L, enc=enc)
            scored = ids.clone()
            open_ = ~(ids[:, 1:-1] == 102).any(1)
            scored[open_, -1] = last[open_]
            seq_lp, tok_lp, _ = OR.token_logprobs_as_written(sd, img, scored, vis[:, j], L, enc=enc)
            for k, v in zip(cols, (ids, mg, last, lp, tok_lp, seq_lp)):
                cols[k].append(v)
        out.update({k: torch.stack(v, 1) for k, v in cols.items()})
    return {k: v.numpy() for k, v in out.items()}


if __name__ == '__main__':      # python tests/region_ref.py: writes tests/golden/region_captions.npz
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
