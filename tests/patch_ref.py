"""Test helper of the patch-removal tests (tests/test_patches_cpu.py, tests/test_hip_patches.py): a torch restatement of the dense
attention with keys removed per image that vitcap_attn_dense_fwd_keys defines (include/vitcap_hip.h) -- with the device's rounding
points and in plain fp32 --, the mask kinds both suites feed it, deliberately wrong variants for the comparator's teeth, and the
oracle's split encoder with patches removed from every ViT block.  Pure torch on the CPU; nothing here touches the GPU library.

The op: image b, heads 12 x 64 over packed qkv (B, S, 2304); key k is visible to EVERY query row of image b iff visible[b, k].  A hidden
key's score is -inf before the row maximum, hidden query rows are computed like the others, and an image without a visible key gives
zero rows."""
import math

import torch

NH, HD, QKV_LD, KT = 12, 64, 2304, 64

MUTATIONS = ('bit0_off_by_one', 'wrong_image', 'leftover_unmasked', 'tail_unmasked')

# the kinds of test 1 of tests/test_hip_patches.py; a kind that needs a tile or a left-over key the shape lacks falls back to 'random'
MASK_KINDS = ('random', 'only_0', 'hide_0', 'hide_last', 'hide_31', 'hide_32', 'hide_63', 'hide_64', 'hide_127', 'hide_128',
              'tile1_hidden', 'only_tile1', 'leftover_hidden', 'only_leftover', 'garbage_past_S')


# the three images of every shape of test 1: together the eight shapes hold every kind on every key path it can reach
OP_KINDS = {5: ('random', 'only_0', 'hide_0'), 40: ('hide_last', 'hide_31', 'hide_32'), 64: ('hide_63', 'hide_0', 'garbage_past_S'),
            130: ('hide_64', 'hide_127', 'hide_128'), 200: ('tile1_hidden', 'leftover_hidden', 'only_leftover'),
            276: ('only_tile1', 'hide_last', 'garbage_past_S'), 577: ('leftover_hidden', 'only_tile1', 'random'),
            578: ('only_leftover', 'hide_last', 'garbage_past_S')}


def key_paths(S):
    """(full 64-key tiles, keys of the peeled tail tile, left-over keys on the vector ALU) as csrc/attn.hip splits S."""
    nfull, rem = S // KT, S % KT
    return nfull, (rem if rem > 8 else 0), (rem if rem <= 8 else 0)


def mask_of_kind(kind, S, gen):
    """bool (S,), True = visible."""
    nfull, tail, left = key_paths(S)
    rnd = torch.rand(S, generator=gen) < 0.5
    rnd[int(torch.randint(S, (1,), generator=gen))] = True           # never empty
    m = torch.ones(S, dtype=torch.bool)
    if kind in ('random', 'garbage_past_S'):
        return rnd
    if kind == 'only_0':
        m[1:] = False
    elif kind == 'hide_last':
        m[S - 1] = False
    elif kind.startswith('hide_'):
        k = int(kind[5:])
        if k >= S:
            return rnd
        m[k] = False
    elif kind in ('tile1_hidden', 'only_tile1'):
        if nfull < 2:
            return rnd
        m[:] = kind == 'tile1_hidden'
        m[KT:2 * KT] = kind != 'tile1_hidden'
    elif kind in ('leftover_hidden', 'only_leftover'):
        if left == 0 or nfull == 0:
            return rnd
        m[:] = kind == 'leftover_hidden'
        m[nfull * KT:] = kind != 'leftover_hidden'
    else:
        raise ValueError(kind)
    return m if bool(m.any()) else rnd


def pack_keys(visible, bit0, garbage=None, extra_words=0):
    """bool (B, S) -> int32 (B, ceil((S + bit0) / 32) + extra_words): key k is bit (k + bit0) & 31 of word (k + bit0) >> 5.  Position 0
    under bit0 = 1 and the positions past the last key are clear, or random where garbage[b] is set (the kernel must ignore them)."""
    visible = torch.as_tensor(visible).bool()
    B, S = visible.shape
    nw = (S + bit0 + 31) // 32 + extra_words
    bits = torch.zeros((B, nw * 32), dtype=torch.int64)
    if garbage is not None:
        g = torch.Generator().manual_seed(4321)
        junk = (torch.rand((B, nw * 32), generator=g) < 0.5).to(torch.int64)
        bits = junk * torch.as_tensor(garbage).view(B, 1).to(torch.int64)
    bits[:, bit0:bit0 + S] = visible.to(torch.int64)
    words = (bits.view(B, nw, 32) << torch.arange(32, dtype=torch.int64)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def _mutated(visible, S, mutate):
    assert mutate is None or mutate in MUTATIONS
    vis = torch.as_tensor(visible).bool().clone()
    nfull, tail, left = key_paths(S)
    if mutate == 'bit0_off_by_one':              # key k reads the bit of key k + 1 (the bit past the last key is clear)
        vis = torch.cat([vis[:, 1:], torch.zeros(vis.shape[0], 1, dtype=torch.bool)], 1)
    if mutate == 'wrong_image':                  # image b reads image b - 1's row
        vis = torch.roll(vis, 1, 0)
    if mutate == 'leftover_unmasked' and left:
        vis[:, nfull * KT:] = True
    if mutate == 'tail_unmasked' and tail:
        vis[:, nfull * KT:] = True
    return vis


def dense_keys_ref(qkv, visible, mutate=None, emulate=True):
    """-> (B, S, 768) fp32.  qkv (B, S, 2304) holding bf16 values, visible bool (B, S).  emulate: the device's rounding points
    (oracle.softmax_pv_rounded with the rounded row sum, as oracle.attn_rounded); otherwise softmax in fp32 with -inf scores."""
    from oracle import vitcap_oracle as O
    qkv = qkv.detach().cpu().float()
    B, S = qkv.shape[:2]
    vis = _mutated(visible, S, mutate)
    q, k, v = qkv.view(B, S, 3, NH, HD).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)).masked_fill(~vis[:, None, None, :], -math.inf)
    out = torch.zeros(B, NH, S, HD)
    live = vis.any(1)                            # an image without a visible key: zero rows (the kernel's guarded normaliser)
    if emulate:
        out[live] = O.softmax_pv_rounded(s[live], v[live], O._R(True), sum_rounded=True)
    else:
        out[live] = torch.softmax(s[live] * 0.125, -1) @ v[live]
    return out.transpose(1, 2).reshape(B, S, 768)


def violations(got, want, rtol=2 ** -7, atol=2e-3):
    """Elements that miss the attention comparator's bound |err| <= atol + rtol |want| -> (count, max |err|)."""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    err = (got - want).abs()
    return int((~(err <= atol + rtol * want.abs())).sum()), float(err.max())


def op_case(S, bit0, seed=None, B=3):
    """Inputs of test 1 for one shape: bf16-valued qkv (B, S, 2304), visible bool (B, S) with a different kind per image, the kinds,
    and which images carry garbage in the bits past S.  Values are uniform in [-1, 1): the bound against the fp32 softmax (4e-3 +
    2^-6 |want|) assumes the bf16 rounding of P (2^-9 relative per term) averages over many keys; with one or two visible keys it does
    not, the error reaches 2 * 2^-9 * max|v| where the terms cancel (want = 0), and max|v| = 1 keeps that below 4e-3."""
    g = torch.Generator().manual_seed(1000 + S if seed is None else seed)
    qkv = (torch.rand((B, S, QKV_LD), generator=g) * 2 - 1).to(torch.bfloat16).float()
    kinds = list(OP_KINDS.get(S, MASK_KINDS[:B]))[:B]
    kinds += ['random'] * (B - len(kinds))
    visible = torch.stack([mask_of_kind(kd, S, g) for kd in kinds])
    garbage = torch.tensor([kd == 'garbage_past_S' for kd in kinds])
    return qkv, visible, kinds, garbage


# ---- the encoder with patches removed: the oracle's split encoder with the reference's additive mask in every block
NVIS, GRID = 578, 24
E2E_MUTATIONS = ('caption_rows_unmasked', 'visual_rows_unmasked')


def vit_attention_removed(sd, p, x, add_mask):
    """oracle.vit_attention with the additive mask Attention.forward receives (vision_transformer.py:174-182): add_mask (B, 1, 1, N),
    0 for a present key and -10000 for a removed one, added to the scaled scores of every query row."""
    from oracle import vitcap_oracle as O
    B, N, C = x.shape
    qkv = O._lin(sd, p + '.qkv', x).reshape(B, N, 3, O.HEADS, C // O.HEADS).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    attn = (q @ k.transpose(-2, -1)) * (O.HD ** -0.5) + add_mask
    attn = attn.softmax(dim=-1)
    x = (attn @ v).transpose(1, 2).reshape(B, N, C)
    return O._lin(sd, p + '.proj', x)


def split_encoder_removed(sd, img_feats, present):
    """oracle.split_encoder (modeling_bert.py:458-478) with removed patches: present bool (B, 578) in cache order (0 tag cls, 1 cls,
    2 + p patch p; both cls set) -- encoder key k is cache key k + 1.  With everything present it is split_encoder exactly."""
    from oracle import vitcap_oracle as O
    present = torch.as_tensor(present).bool()
    assert tuple(present.shape) == (img_feats.shape[0], NVIS) and bool(present[:, :2].all())
    add = ((~present[:, 1:]).to(img_feats.dtype) * -10000.0)[:, None, None, :]

    def block(p, x):
        x = x + vit_attention_removed(sd, p + '.attn', O._ln(sd, p + '.norm1', x, 1e-6), add)
        return x + O.vit_mlp(sd, p + '.mlp', O._ln(sd, p + '.norm2', x, 1e-6))

    h, tag_h = img_feats, None
    for i in range(12):
        if i == 8:
            tag_h = h
        h = block('module.bert.encoder.blocks.%d' % i, h)
    for i in range(4):
        tag_h = block('module.bert.encoder.tag_blocks.%d' % i, tag_h)
    return h, tag_h


def prefill_rows_removed(sd, enc, present, mutate=None):
    """The decoder's visual rows after layers 0..2 -- what the engine's prefill keeps as the input of the last layer's K/V
    (vitcap_engine_tap 'vis') -- with the removed keys' columns at -10000: (B, 578, 768) in cache order.  Visual rows attend visual
    rows only (the zero block of construct_attn_mask), so the caption does not enter.  mutate 'visual_rows_unmasked': no removal here."""
    from oracle import vitcap_oracle as O
    hidden, tag_hidden = enc
    x = torch.cat([tag_hidden[:, :1], hidden], 1)
    keep = torch.as_tensor(present).to(x.dtype)
    if mutate == 'visual_rows_unmasked':
        keep = torch.ones_like(keep)
    ext = (1.0 - keep)[:, None, None, :] * -10000.0
    for i in range(3):
        x = O.bert_layer(sd, 'module.bert.decoder.layer.%d' % i, x, ext, None, 0.0, None, 0.0)
    return x


def _steps(sd, image, present, max_length, given=None, mutate=None, enc=None):
    """The as-written loop (oracle.greedy_as_written / sequence_logprob_as_written: one full forward per position on [tokens so far,
    MASK, tag slots]) on the encoder with `present`'s patches removed and the removed keys' columns zero for ALL rows of the joint
    mask -- caption, tag-slot and visual rows; key 577 through the `last_col` device of occlusion_ref.joint_forward_masked.
    given None: greedy; else ids (B, L) to score.  mutate: the removal is left out of the caption rows / of the visual rows."""
    import torch.nn.functional as F

    import occlusion_ref as OR
    from oracle import vitcap_oracle as O
    assert mutate is None or mutate in E2E_MUTATIONS
    B = image.shape[0]
    present = torch.as_tensor(present).bool()
    img_feats = O.patch_embed(sd, image)
    input_ids0, am = O.test_text_inputs(B, max_length)
    full_mask = O.construct_attn_mask(am, img_feats.shape[1])
    od_label_ids = input_ids0[:, max_length:]
    od_len = od_label_ids.shape[1]
    full_pos = torch.arange(max_length + od_len).unsqueeze(0).expand(B, -1)
    full_tt = torch.zeros(B, max_length + od_len, dtype=torch.long)
    if enc is None:
        enc = split_encoder_removed(sd, img_feats, present)
    ids = torch.full((B, 1), O.BOS, dtype=torch.long)
    unfinished = torch.ones(B)
    tok_lp, cnt = torch.zeros(B, max_length), torch.zeros(B)
    margins = torch.full((B, max_length - 1), float('inf'))
    nxt = None
    for cur_len in range(1, max_length):
        step_ids = torch.cat([ids if given is None else given[:, :cur_len], torch.full((B, 1), O.MASK, dtype=torch.long)], dim=1)
        curr = step_ids.shape[1]
        mask = O._remove_rows_cols(full_mask, curr, max_length, curr, max_length).clone()
        T = curr + od_len
        rows = mask.shape[1] + 1                                   # joint_forward_masked appends the last visual row
        keep = torch.ones(B, rows, NVIS)
        keep *= present[:, None, :].to(keep.dtype)
        if mutate == 'caption_rows_unmasked':
            keep[:, :curr] = 1
        if mutate == 'visual_rows_unmasked':
            keep[:, T:] = 1
        mask[:, :, T:] *= keep[:, :rows - 1, :NVIS - 1]
        last_col = keep[:, :, NVIS - 1] * torch.cat([torch.ones(B, curr), torch.zeros(B, od_len), torch.ones(B, rows - T)], 1)
        tt = torch.cat([full_tt[:, :curr], full_tt[:, max_length:]], dim=1)
        pp = torch.cat([full_pos[:, :curr], full_pos[:, max_length:]], dim=1)
        seq = OR.joint_forward_masked(sd, torch.cat([step_ids, od_label_ids], dim=1), mask, last_col, pp, tt, enc)
        logits = O.lm_head(sd, 'module.cls', seq[:, cur_len:cur_len + 1])[:, 0]
        top2 = logits.topk(2, dim=-1)
        nxt = top2.indices[:, 0]
        tok = nxt if given is None else given[:, cur_len]
        live = unfinished.bool()
        margins[live, cur_len - 1] = (top2.values[:, 0] - top2.values[:, 1])[live]
        lp = torch.gather(F.log_softmax(logits, dim=-1), -1, tok.unsqueeze(-1)).squeeze(-1)
        tok_lp[:, cur_len] = lp * unfinished
        cnt += unfinished
        add = (tok * unfinished.long() + O.PAD * (1 - unfinished.long())) if given is None else tok
        ids = torch.cat([ids, add.unsqueeze(-1)], dim=-1)
        unfinished = unfinished * tok.ne(O.EOS).float()
    if given is None:
        ids[:, -1].masked_fill_(unfinished.bool(), O.EOS)
    return ids, tok_lp.sum(1) / cnt, tok_lp, margins, nxt, enc


def greedy_removed(sd, image, present, max_length, mutate=None, enc=None):
    """-> (ids (B, L), logprob (B,), margins (B, L - 1), last (B,): the token chosen at the last position, enc)."""
    ids, lp, _, margins, last, enc = _steps(sd, image, present, max_length, None, mutate, enc)
    return ids, lp, margins, last, enc


def token_logprobs_removed(sd, image, ids, present, max_length, mutate=None, enc=None):
    """-> (logprob (B,), token_logprobs (B, L)) of the GIVEN captions."""
    _, lp, tok_lp, _, _, _ = _steps(sd, image, present, max_length, ids, mutate, enc)
    return lp, tok_lp


# ---- the end-to-end case of tests/test_hip_patches.py tests 6 and 7, chosen in the reference alone
CASE_L, CASE_SEED = 8, 1234          # the images and max_length of tests/test_hip_regions.py's end-to-end test
CASE_BOXES = ((9, 9, 15, 15), (0, 0, 6, 6))      # mask 0: all patches but a 6 x 6 box removed (image 0 central, image 1 top-left)
CASE_FILE = 'patch_removal.npz'      # under tests/golden: the reference's results for the case, so that the GPU test computes none


def case_inputs():
    """-> (images (2, 3, 384, 384), present bool (2, 3, 578)): per image mask 0 = only its box of CASE_BOXES, mask 1 = the upper half
    of the image (patch rows 0..11), mask 2 = everything (the control); both cls keys always."""
    from vitcap_amd import regions as RG
    from vitcap_amd import weights as W
    img = torch.from_numpy(W.gen_image_batch(2, CASE_SEED))
    pres = torch.ones(2, 3, NVIS, dtype=torch.bool)
    pres[:, 0] = RG.box_masks(torch.tensor(CASE_BOXES))
    pres[:, 1, 2 + 12 * GRID:] = False
    return img, pres


def build_case(sd):
    """The reference's own results for the case, as numpy arrays, per image and mask (2, 3, ...): digests of the encoder's outputs
    (hidden (577, 768) and tag_hidden[:, 0] as fp32 arrays -- small enough to keep whole for the two CLS rows, `hidden` as its
    per-row L2 norms and the rows of 8 probe patches), the tag logits' first 64 and top 50, the same digest of the decoder's visual
    rows after the prefill (prefill_rows_removed), the greedy ids, margins, last choice and log-prob, and the per-token log-probs of
    those captions."""
    from oracle import vitcap_oracle as O
    img, pres = case_inputs()
    L = CASE_L
    cols = {k: [] for k in ('hidden_norms', 'hidden_probe', 'tag_cls', 'tag_logits64', 'tag_logits_max', 'tag_topk', 'tag_prob', 'tag_len',
                            'vis_norms', 'vis_probe', 'ids', 'margins', 'last', 'greedy_lp', 'tok_lp', 'seq_lp')}
    with torch.no_grad():
        for j in range(pres.shape[1]):
            ids, lp, mg, last, enc = greedy_removed(sd, img, pres[:, j], L)
            hidden, tag_hidden = enc
            logit, prob, topk, tlen = O.tag_head(sd, tag_hidden, 50)
            scored = ids.clone()
            open_ = ~(ids[:, 1:-1] == 102).any(1)
            scored[open_, -1] = last[open_]
            seq_lp, tok_lp = token_logprobs_removed(sd, img, scored, pres[:, j], L, enc=enc)
            vis = prefill_rows_removed(sd, enc, pres[:, j])
            vals = (hidden.norm(dim=-1), hidden[:, PROBE_ROWS], tag_hidden[:, 0], logit[:, :64], logit.abs().max(1).values, topk, prob, tlen,
                    vis.norm(dim=-1), vis[:, VIS_PROBE_ROWS], ids, mg, last, lp, tok_lp, seq_lp)
            for k, v in zip(cols, vals):
                cols[k].append(v)
    return {k: torch.stack(v, 1).numpy() for k, v in cols.items()}


# rows of `hidden` (encoder order: 0 cls, 1 + p patch p) kept whole in the case file: cls, the corners and centre of both boxes
PROBE_ROWS = [0, 1, 1 + 5 * GRID + 5, 1 + 9 * GRID + 9, 1 + 12 * GRID + 12, 1 + 14 * GRID + 14, 1 + 11 * GRID + 23, 576]
VIS_PROBE_ROWS = [0] + [r + 1 for r in PROBE_ROWS[:7]]      # cache order: the tag cls, then the same rows (the last probe left out)
# probes that are PRESENT under mask 0 / mask 1 of the case, per image, as indices into PROBE_ROWS (cls; patches (9,9) (12,12) (14,14)
# in image 0's box, (0,0) (5,5) in image 1's; (0,0) (5,5) (9,9) (11,23) in the upper half)
PRESENT_PROBES = {(0, 0): [0, 3, 4, 5], (1, 0): [0, 1, 2], (0, 1): [0, 1, 2, 3, 6], (1, 1): [0, 1, 2, 3, 6]}


if __name__ == '__main__':      # python tests/patch_ref.py: writes tests/golden/patch_removal.npz
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
        print(k, v.shape, v.reshape(-1)[:8].tolist())
