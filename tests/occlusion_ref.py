"""Test helper of the occlusion tests (tests/test_occlusion_cpu.py, tests/test_hip_occlusion.py): a torch restatement of the masked
text-grid attention that vitcap_attn_text_grid_masked defines (include/vitcap_hip.h) -- in fp64, and in the rounding-emulated form
tests/test_hip_score_onepass.py compares vitcap_attn_text_grid with --, the masks and planted inputs both suites feed it, deliberately
wrong variants for the comparator's teeth, and the end-to-end reference: the oracle's joint forward looped over cur_len with the hidden
visual columns zeroed in the caption rows of the joint attention mask.  Pure torch on the CPU; nothing here touches the GPU library.

The op: caption c of image c // K, grid rows r = 0..2L-2 (token rows 0..L-1, probe j at row L + j).  Keys: the image's 578 visual rows,
visible to every row of the caption where bit k of the caption's mask is set, then the caption's own grid rows under the grid mask
(token row r: tokens <= r; probe j: tokens 0..j and itself), which the visibility mask never touches."""
import math

import torch

import attn_maps_ref as AR

NVIS, NH, HD, QKV_LD = 578, 12, 64, 2304
C_LOG2 = 0.125 * 1.4426950408889634

MUTATIONS = ('bit_shift', 'wrong_caption', 'token_masked', 'probe_rows_only')

# the kinds of test 2 of tests/test_hip_occlusion.py, in the order the captions take them
MASK_KINDS = ('random', 'all_hidden', 'only_0', 'only_577', 'hide_16_31', 'bit_15', 'bit_16', 'bit_31', 'bit_32', 'bit_575', 'bit_576',
              'bit_577')


def mask_of_kind(kind, gen):
    """bool (578,), True = visible."""
    if kind == 'random':
        return torch.rand(NVIS, generator=gen) < 0.5
    m = torch.ones(NVIS, dtype=torch.bool)
    if kind == 'all_hidden':
        m[:] = False
    elif kind.startswith('only_'):
        m[:] = False
        m[int(kind[5:])] = True
    elif kind == 'hide_16_31':
        m[16:32] = False
    else:
        m[int(kind[4:])] = False
    return m


def masks_by_kind(n_caps, seed):
    """bool (n_caps, 578): caption i takes kind i % 12, so that with 9 captions per image the two images of a batch hold different
    masks and every kind appears among 18 captions; the random ones differ per caption."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([mask_of_kind(MASK_KINDS[i % len(MASK_KINDS)], g) for i in range(n_caps)])


def grid_mask(L):
    """(R, R) bool: text key k visible to grid row r."""
    R = 2 * L - 1
    m = torch.zeros(R, R, dtype=torch.bool)
    for r in range(R):
        m[r, :(r if r < L else r - L) + 1] = True
        if r >= L:
            m[r, r] = True
    return m


def _visible_scores_mask(visible, n_img, K, L, mutate):
    """(NC, R, 578 + R) bool: what row r of caption c may attend, with the mutation applied."""
    assert mutate is None or mutate in MUTATIONS
    R, NC = 2 * L - 1, n_img * K
    vis = torch.as_tensor(visible).bool().clone()
    assert tuple(vis.shape) == (NC, NVIS)
    if mutate == 'bit_shift':                    # key k reads bit k + 1 (bit 578 is a clear padding bit)
        vis = torch.cat([vis[:, 1:], torch.zeros(NC, 1, dtype=torch.bool)], 1)
    if mutate == 'wrong_caption':                # caption c reads caption c - 1's mask (caption 0 the last one's)
        vis = torch.roll(vis, 1, 0)
    allow = torch.ones(NC, R, NVIS + R, dtype=torch.bool)
    allow[:, :, :NVIS] = vis[:, None, :]
    if mutate == 'probe_rows_only':              # token rows see every visual key
        allow[:, :L, :NVIS] = True
    allow[:, :, NVIS:] = grid_mask(L)
    if mutate == 'token_masked':                 # token key k also obeys bit k
        allow[:, :, NVIS:NVIS + L] &= vis[:, None, :L]
    return allow


def masked_grid_ref(qkv_text, vis_qkv, visible, n_img, K, L, mutate=None, emulate=True):
    """-> (NC, R, 768).  qkv_text bf16 (NC * R, 2304), vis_qkv bf16 (n_img * 578, 2304), visible bool (NC, 578).
    emulate: the device's rounding points (oracle.softmax_pv_rounded: fp32 scores, m = ceil(max * c), bf16 P for the product, the
    row sum from the unrounded P), fp32 result; otherwise the same mathematics in float64."""
    R, NC = 2 * L - 1, n_img * K
    dt = torch.float32 if emulate else torch.float64
    x = qkv_text.detach().cpu().to(dt).view(NC, R, QKV_LD)
    v = vis_qkv.detach().cpu().to(dt).view(n_img, NVIS, QKV_LD).repeat_interleave(K, 0)
    Kk = torch.cat([v[..., 768:1536], x[..., 768:1536]], 1).view(NC, NVIS + R, NH, HD).transpose(1, 2)
    Vv = torch.cat([v[..., 1536:], x[..., 1536:]], 1).view(NC, NVIS + R, NH, HD).transpose(1, 2)
    q = x[..., :768].reshape(NC, R, NH, HD).transpose(1, 2)
    s = q @ Kk.transpose(-1, -2)                                                  # (NC, 12, R, 578 + R)
    allow = _visible_scores_mask(visible, n_img, K, L, mutate)
    s = s.masked_fill(~allow[:, None], -math.inf)
    if emulate:
        from oracle import vitcap_oracle as O
        o = O.softmax_pv_rounded(s, Vv, O._R(True))
    else:
        m = torch.ceil(s.max(-1, keepdim=True).values * C_LOG2)
        p = torch.exp2(s * C_LOG2 - m)
        o = (p @ Vv) / p.sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(NC, R, 768)


def violations(got, want):
    """Elements that miss the attention comparator's bound |err| <= 2e-3 + 2^-7 |want| -> (count, max |err|)."""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    err = (got - want).abs()
    return int((err > 2e-3 + 2 ** -7 * want.abs()).sum()), float(err.max())


# ---- planted inputs: keys that dominate a row, so that hiding them visibly moves it
PLANT_TOKEN_ROW, PLANT_TOKEN_HEAD, PLANT_PROBE_HEAD = 2, 4, 2
EXTRA_HIDDEN = 3          # one more hidden visual key: token key 3 dominates probe 4 in head 3, which 'token_masked' then hides too
MOVE_THRESHOLD = 0.5      # a (row, head) slice "moved" when some element changes by more than this (see planted_inputs)


def planted_probe_key(c, t):
    return (37 * t + 5 * c) % NVIS


def planted_token_key(c):
    return 400 + 7 * c


def planted_inputs(n_img, K, L, seed):
    """attn_maps_ref.make_inputs(planted=True), reworked so that the mask moves the planted slices and nothing else:
      * per caption c and probe t = 1, 4, 7, .. visual key (37 t + 5 c) % 578 (make_inputs' own choice) is TWICE the probe's q in
        head 2 and zero in every other head; per caption, visual key 400 + 7 c is twice TOKEN row 2's q in head 4 and zero elsewhere,
        so that token rows depend on the mask too;
      * every other row of the caption has q = 0 in head 2, and every row but token row 2 has q = 0 in head 4; visual key
        EXTRA_HIDDEN is zero in all heads.
    A planted key scores 2 |q|^2 / 8 = 16 +- 3 against N(0, 1) for each of the other 600 keys: even at 9.5 it holds e^9.5 / (e^9.5 +
    600 e^0.5) > 0.9 of its row, so hiding it moves that row's head slice by about 0.9 max|v| (64 elements of N(0, 1): above 1.5),
    far above MOVE_THRESHOLD.  Everywhere else a hidden key scores exactly 0 -- a weight of about 1 / 600 -- and the five hidden
    keys together move a slice by about 0.01, far below it.
    -> (qkv_text, vis_qkv, visible bool (NC, 578): caption c hides its own planted keys and key EXTRA_HIDDEN,
        planted: the set of (caption, grid row, head) whose slice the mask moves)."""
    assert n_img * K <= 18 and 6 <= L <= 8          # the planted key indices stay distinct: probes 37..344, tokens 400..519
    x, v = AR.make_inputs(n_img, K, L, seed, planted=True)
    R, NC = 2 * L - 1, n_img * K
    x, v = x.view(NC, R, QKV_LD).clone(), v.view(n_img, NVIS, QKV_LD).clone()
    visible = torch.ones(NC, NVIS, dtype=torch.bool)
    planted = set()
    hp, ht = PLANT_PROBE_HEAD, PLANT_TOKEN_HEAD
    v[:, EXTRA_HIDDEN, 768:1536] = 0
    for c in range(NC):
        probes = [L + t - 1 for t in range(1, L, 3)]
        for r in range(R):
            if r not in probes:
                x[c, r, hp * HD:(hp + 1) * HD] = 0
            if r != PLANT_TOKEN_ROW:
                x[c, r, ht * HD:(ht + 1) * HD] = 0
        k = planted_token_key(c)
        v[c // K, k, 768:1536] = 0
        v[c // K, k, 768 + ht * HD:768 + (ht + 1) * HD] = 2 * x[c, PLANT_TOKEN_ROW, ht * HD:(ht + 1) * HD]
        visible[c, k] = False
        planted.add((c, PLANT_TOKEN_ROW, ht))
        for t in range(1, L, 3):
            k = planted_probe_key(c, t)
            v[c // K, k, 768:1536] = 0
            v[c // K, k, 768 + hp * HD:768 + (hp + 1) * HD] = 2 * x[c, L + t - 1, hp * HD:(hp + 1) * HD]
            visible[c, k] = False
            planted.add((c, L + t - 1, hp))
        visible[c, EXTRA_HIDDEN] = False
    return x.view(NC * R, QKV_LD), v.view(n_img * NVIS, QKV_LD), visible, planted


def moved(a, b, L):
    """The (caption, grid row, head) slices in which (NC, R, 768) arrays a and b differ by more than MOVE_THRESHOLD somewhere
    (token row L - 1, which feeds nothing, left out) -> (set, smallest move inside the set, largest outside)."""
    d = (torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs()
    d = d.view(d.shape[0], d.shape[1], NH, HD).max(-1).values
    d[:, L - 1] = 0
    hit = d > MOVE_THRESHOLD
    inside = float(d[hit].min()) if bool(hit.any()) else float('nan')
    outside = float(d[~hit].max())
    return set(map(tuple, hit.nonzero().tolist())), inside, outside


# ---- end to end: the oracle's forward as written, with visual columns hidden from the caption rows
def joint_forward_masked(sd, input_ids, attention_mask, last_col, position_ids, token_type_ids, enc):
    """oracle.vitcap_oracle.joint_forward (tagemb = 'cls', no dropout, the encoder precomputed) with ONE difference: the column the
    forward appends to the mask for the last visual row (key 577; modeling_bert.py:1498-1499 pads it with ones) is `last_col`
    (B, rows + 1) instead of ones, so that key 577 can be hidden as well.  attention_mask (B, S - 1, S - 1) as joint_forward takes
    it.  -> sequence_output (B, S, 768)."""
    from oracle import vitcap_oracle as O
    input_ids = input_ids.clone()
    hidden, tag_hidden = enc
    logit, prob, pred_topk, topk_len = O.tag_head(sd, tag_hidden, 50)
    pred_topk = pred_topk.clone()
    cls_w = sd['module.cls.predictions.decoder.weight']
    T = input_ids.shape[1]
    if int(topk_len[0]) + 20 <= T:
        pred_topk[:, -1] = O.EOS
        emb = O.bert_embeddings(sd, 'module.bert.embeddings', input_ids, position_ids, token_type_ids)
        tag_emb = cls_w[pred_topk]
    else:
        input_ids[:, T - topk_len] = O.EOS
        pred_topk[:, -1] = O.EOS
        tag_emb = O.encode_tag_to_embedding(sd, pred_topk, cls_w)
        emb = O.bert_embeddings(sd, 'module.bert.embeddings', input_ids, position_ids, token_type_ids)
    emb[:, -pred_topk.shape[1]:] = tag_emb
    enc_out = torch.cat([tag_hidden[:, 0, :].unsqueeze(1), hidden], 1)
    am = torch.cat([attention_mask, attention_mask[:, -1].unsqueeze(1)], dim=1)
    am = torch.cat([am, last_col.unsqueeze(2)], dim=2)
    ext = (1.0 - am.unsqueeze(1)) * -10000.0
    x = torch.cat((emb, enc_out), 1)
    for i in range(4):
        x = O.bert_layer(sd, 'module.bert.decoder.layer.%d' % i, x, ext, None, 0.0, None, 0.0)
    return x


def token_logprobs_as_written(sd, image, ids, visible, max_length, enc=None):
    """Per-token log-probs of GIVEN captions the way oracle.sequence_logprob_as_written computes them -- one full forward per position
    on [tokens so far, MASK, tag slots], log_softmax gathered at the given token, the unfinished averaging -- with the visual columns
    where `visible` (B, 578) is False zeroed in the caption rows (the tokens so far and the MASK) of the joint mask.  ids (B, L):
    the tokens to score at positions 1..L-1.  -> (logprob (B,), token_logprobs (B, L), enc) in the oracle's fp32."""
    import torch.nn.functional as F
    from oracle import vitcap_oracle as O
    B = image.shape[0]
    visible = torch.as_tensor(visible).bool()
    img_feats = O.patch_embed(sd, image)
    input_ids0, am = O.test_text_inputs(B, max_length)
    full_mask = O.construct_attn_mask(am, img_feats.shape[1])              # (B, T + 577, T + 577)
    od_label_ids = input_ids0[:, max_length:]
    od_len = od_label_ids.shape[1]
    full_pos = torch.arange(max_length + od_len).unsqueeze(0).expand(B, -1)
    full_tt = torch.zeros(B, max_length + od_len, dtype=torch.long)
    if enc is None:
        enc = O.split_encoder(sd, img_feats)
    unfinished = torch.ones(B)
    tok_lp = torch.zeros(B, max_length)
    cnt = torch.zeros(B)
    for cur_len in range(1, max_length):
        step_ids = torch.cat([ids[:, :cur_len], torch.full((B, 1), O.MASK, dtype=torch.long)], dim=1)
        curr = step_ids.shape[1]
        mask = O._remove_rows_cols(full_mask, curr, max_length, curr, max_length).clone()
        T = curr + od_len
        mask[:, :curr, T:] *= visible[:, None, :NVIS - 1].to(mask.dtype)    # visual keys 0..576 of the caption rows
        last_col = torch.ones(B, mask.shape[1] + 1)
        last_col[:, :curr] = visible[:, NVIS - 1:].to(mask.dtype)           # key 577, the appended column
        tt = torch.cat([full_tt[:, :curr], full_tt[:, max_length:]], dim=1)
        pp = torch.cat([full_pos[:, :curr], full_pos[:, max_length:]], dim=1)
        seq = joint_forward_masked(sd, torch.cat([step_ids, od_label_ids], dim=1), mask, last_col, pp, tt, enc)
        logits = O.lm_head(sd, 'module.cls', seq[:, cur_len:cur_len + 1])[:, 0]
        tok = ids[:, cur_len]
        lp = torch.gather(F.log_softmax(logits, dim=-1), -1, tok.unsqueeze(-1)).squeeze(-1)
        tok_lp[:, cur_len] = lp * unfinished
        cnt += unfinished
        unfinished = unfinished * tok.ne(O.EOS).float()
    return tok_lp.sum(1) / cnt, tok_lp, enc
