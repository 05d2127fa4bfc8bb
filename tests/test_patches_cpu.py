"""Patch removal without a GPU: the torch restatement of tests/patch_ref.py against the reference's own encoder and tag head under
removal masks (tests/golden/reference_patches.npz, written by tests/golden/make_golden_patches.py from the reference), the committed
end-to-end case (tests/golden/patch_removal.npz) recomputed, the comparator's teeth (every deliberately wrong variant is flagged), the
host helpers of vitcap_amd/patches.py and every refusal of the Python surface."""
import os

import numpy as np
import pytest
import torch

import patch_ref as PR

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(5, 0), (40, 1), (64, 0), (130, 0), (200, 1), (276, 0), (577, 1), (578, 0)]
TOK_TOL = 4e-2          # tests/test_hip_regions.py: the per-token bound of the end-to-end comparison


@pytest.fixture(scope='module')
def case(sd_t):
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    return PR.build_case(sd_t)


# ------------------------------------------------------------------------------------------------ the op's restatement
def test_restated_attention_is_the_softmax_over_the_visible_keys():
    """-inf scores give no NaN, and the result is the softmax over the gathered visible keys (fp32: to 2e-6; the emulation within
    its bound of it)."""
    qkv, visible, _, _ = PR.op_case(130, 0)
    ref = PR.dense_keys_ref(qkv, visible, emulate=False)
    emu = PR.dense_keys_ref(qkv, visible)
    assert not bool(torch.isnan(ref).any() | torch.isnan(emu).any())
    for b in range(3):
        keep = visible[b].nonzero().flatten()
        q, k, v = qkv[b].view(130, 3, 12, 64).permute(1, 2, 0, 3)
        want = (torch.softmax(q @ k[:, keep].transpose(-1, -2) * 0.125, -1) @ v[:, keep]).transpose(0, 1).reshape(130, 768)
        assert float((ref[b] - want).abs().max()) < 2e-6
    assert PR.violations(emu, ref, 2 ** -6, 4e-3)[0] == 0
    dead = visible.clone()
    dead[1] = False
    out = PR.dense_keys_ref(qkv, dead)
    assert bool((out[1] == 0).all()) and torch.equal(out[0], emu[0])


def test_every_wrong_variant_of_the_op_is_flagged():
    """Each mutant misses the comparator's bound on at least one of test 1's shapes, and the shapes together hold every mask kind."""
    flagged = {m: 0 for m in PR.MUTATIONS}
    kinds = set()
    for S, bit0 in SHAPES:
        qkv, visible, kd, _ = PR.op_case(S, bit0)
        kinds |= set(kd)
        want = PR.dense_keys_ref(qkv, visible)
        for m in PR.MUTATIONS:
            flagged[m] += int(PR.violations(PR.dense_keys_ref(qkv, visible, m), want)[0] > 0)
    assert all(n > 0 for n in flagged.values()), flagged
    assert kinds == set(PR.MASK_KINDS), set(PR.MASK_KINDS) - kinds


def test_pack_keys_layout():
    vis = torch.zeros(2, 70, dtype=torch.bool)
    vis[0, 0] = vis[0, 31] = vis[0, 32] = vis[1, 69] = True
    w0, w1 = PR.pack_keys(vis, 0), PR.pack_keys(vis, 1)
    assert tuple(w0.shape) == (2, 3) and tuple(w1.shape) == (2, 3)
    u = lambda w: [[int(x) & 0xFFFFFFFF for x in r] for r in w.tolist()]      # noqa: E731
    assert u(w0) == [[0x80000001, 1, 0], [0, 0, 1 << 5]]
    assert u(w1) == [[2, 3, 0], [0, 0, 1 << 6]]
    junk = PR.pack_keys(vis, 1, garbage=torch.tensor([True, False]), extra_words=1)
    assert tuple(junk.shape) == (2, 4) and u(junk)[1] == [0, 0, 1 << 6, 0] and u(junk)[0][3] != 0


# ------------------------------------------------------------------------------------------------ the encoder against the reference
def test_everything_present_is_the_oracles_encoder(sd_t):
    from oracle import vitcap_oracle as O
    from vitcap_amd import weights as W
    img = torch.from_numpy(W.gen_image_batch(1, PR.CASE_SEED))
    with torch.no_grad():
        feats = O.patch_embed(sd_t, img)
        a = PR.split_encoder_removed(sd_t, feats, torch.ones(1, PR.NVIS, dtype=torch.bool))
        b = O.split_encoder(sd_t, feats)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_restatement_reproduces_the_reference_under_removal(sd_t):
    """reference_patches.npz holds what the reference's own model.bert.encoder / pooler / tag_logit gave under two removal masks."""
    from oracle import vitcap_oracle as O
    from vitcap_amd import weights as W
    gold = np.load(os.path.join(HERE, 'golden', 'reference_patches.npz'))
    pres = torch.from_numpy(gold['present'])
    img = torch.from_numpy(W.gen_image_batch(2, PR.CASE_SEED))
    with torch.no_grad():
        feats = O.patch_embed(sd_t, img)
        for j in range(pres.shape[1]):
            hid, tag_hid = PR.split_encoder_removed(sd_t, feats, pres[:, j])
            logit, prob, topk, tlen = O.tag_head(sd_t, tag_hid, 50)
            for name, got, tol in (('hidden_norms', hid.norm(dim=-1), 2e-4), ('hidden_probe', hid[:, PR.PROBE_ROWS], 1e-4),
                                   ('tag_cls', tag_hid[:, 0], 1e-4), ('tag_logits64', logit[:, :64], 1e-4),
                                   ('tag_logits_max', logit.abs().max(1).values, 1e-4), ('tag_prob', prob, 1e-5)):
                err = float((got - torch.from_numpy(gold[name][:, j])).abs().max())
                print('MEASURED restatement vs reference, mask %d, %s: max |d| %.3e' % (j, name, err))
                assert err < tol, (j, name, err)
            assert np.array_equal(topk.numpy(), gold['tag_topk'][:, j]) and np.array_equal(tlen.numpy(), gold['tag_len'][:, j])


# ------------------------------------------------------------------------------------------------ the committed end-to-end case
def test_committed_case_is_recomputed(case):
    gold = np.load(os.path.join(HERE, 'golden', PR.CASE_FILE))
    assert set(gold.files) == set(case)
    for k, v in case.items():
        if v.dtype.kind in 'iu':
            assert np.array_equal(v, gold[k]), k
        else:
            fin = np.isfinite(v)
            assert np.array_equal(fin, np.isfinite(gold[k])) and np.allclose(v[fin], gold[k][fin], rtol=1e-4, atol=1e-4), k
    # the control (mask 2: everything present) is the unmasked case of tests/golden/region_captions.npz
    assert np.array_equal(case['ids'][:, 2], np.load(os.path.join(HERE, 'golden', 'region_captions.npz'))['unmasked_ids'])


def test_removal_moves_the_tagger_far_above_the_parity_bound(case):
    """Removing all patches but a 6 x 6 box moves the tag logits by more than 10 x the 2e-2 parity bound, the top-50 set and the
    present rows of `hidden` (relative L2 over the probe rows inside the boxes)."""
    moved = np.abs(case['tag_logits64'][:, 0] - case['tag_logits64'][:, 2]).max()
    changed = [50 - len(set(case['tag_topk'][b, 0]) & set(case['tag_topk'][b, 2])) for b in range(2)]
    rows = {0: [3, 4, 5], 1: [2]}                  # PROBE_ROWS inside image b's box (encoder rows of patches (9,9) (12,12) (14,14); (5,5))
    rel = [float(np.linalg.norm(case['hidden_probe'][b, 0, r] - case['hidden_probe'][b, 2, r]) / np.linalg.norm(case['hidden_probe'][b, 2, r]))
           for b in range(2) for r in rows[b]]
    print('MEASURED removal (6 x 6 box kept): tag logits move by %.3f, top-50 changed %s of 50, present rows of hidden rel L2 %s'
          % (moved, changed, ['%.3f' % x for x in rel]))
    assert moved > 10 * 2e-2 and min(changed) >= 10 and min(rel) > 10 * 1.2e-2


def test_case_margins_leave_enough_whole_captions(case):
    """At least 3 of the 4 removed-patch captions are comparable as a whole (every decision above GREEDY_MARGIN_FLOOR)."""
    from conftest import GREEDY_MARGIN_FLOOR, relevant_margins
    whole = 0
    for b in range(2):
        for j in range(2):
            whole += int(relevant_margins(case['ids'][b, j], case['margins'][b, j], 102).min() >= GREEDY_MARGIN_FLOOR)
    assert whole >= 3, whole


def test_unmasked_visual_rows_are_flagged_by_the_prefill_digest(sd_t, case):
    """A prefill that ignores the removal moves the captions' log-probs by less than the end-to-end bound on this model (measured:
    1.2e-2 per token against 4e-2), so the scores cannot see it; the digest of the decoder's visual rows does: the PRESENT probe rows
    move by several times the 1.2e-2 relative-L2 bound (measured: 0.06) tests/test_hip_patches.py holds the device's rows to."""
    from oracle import vitcap_oracle as O
    img, pres = PR.case_inputs()
    with torch.no_grad():
        enc = PR.split_encoder_removed(sd_t, O.patch_embed(sd_t, img), pres[:, 0])
        good = PR.prefill_rows_removed(sd_t, enc, pres[:, 0])[:, PR.VIS_PROBE_ROWS]
        bad = PR.prefill_rows_removed(sd_t, enc, pres[:, 0], 'visual_rows_unmasked')[:, PR.VIS_PROBE_ROWS]
    assert float((good - torch.from_numpy(case['vis_probe'][:, 0])).abs().max()) < 1e-4
    for b in range(2):
        rows = [i + 1 for i in PR.PRESENT_PROBES[(b, 0)] if i + 1 < len(PR.VIS_PROBE_ROWS)]
        rel = float((bad[b, rows] - good[b, rows]).norm() / good[b, rows].norm())
        print('MEASURED visual_rows_unmasked, image %d: present probe rows of the prefill move by rel L2 %.3f (bound 1.2e-2)' % (b, rel))
        assert rel > 3 * 1.2e-2              # flagged with room: the device's own error is held below 1.2e-2


def test_unmasked_caption_rows_are_flagged_by_the_scores(sd_t, case, mutate='caption_rows_unmasked'):
    """Leaving the removal out of the caption rows moves the per-token log-probs of the committed captions by more than the
    end-to-end bound (mask 0, the encoder recomputed under the mask)."""
    img, pres = PR.case_inputs()
    ids = torch.from_numpy(case['ids'][:, 0]).clone()
    last = torch.from_numpy(case['last'][:, 0])
    open_ = ~(ids[:, 1:-1] == 102).any(1)
    ids[open_, -1] = last[open_]
    with torch.no_grad():
        _, tok = PR.token_logprobs_removed(sd_t, img, ids, pres[:, 0], PR.CASE_L, mutate=mutate)
    d = float((tok - torch.from_numpy(case['tok_lp'][:, 0])).abs().max())
    print('MEASURED %s: per-token log-probs move by %.3e (bound %.1e)' % (mutate, d, TOK_TOL))
    assert d > TOK_TOL


# ------------------------------------------------------------------------------------------------ helpers and refusals
def test_present_helpers():
    from vitcap_amd import patches as P
    from vitcap_amd.occlusion import pack_visible
    from vitcap_amd.regions import grid_regions
    g = torch.zeros(2, 24, 24, dtype=torch.bool)
    g[0, 0, 0] = g[1, 23, 23] = True
    full = P.as_present(g, 2)
    assert tuple(full.shape) == (2, 578) and bool(full[:, :2].all()) and bool(full[0, 2]) and bool(full[1, 577]) and int(full.sum()) == 6
    assert torch.equal(P.as_present(g.reshape(2, 576), 2), full) and torch.equal(P.as_present(full, 2), full)
    assert torch.equal(P.as_present(g.to(torch.uint8), 2), full)
    assert torch.equal(P.pack_present(g, 2), pack_visible(full)) and tuple(P.pack_present(g, 2).shape) == (2, 19)
    for bad, why in ((g.float(), 'bool or uint8'), (g[:1], r'must be \(2, 24, 24\)'), (torch.zeros(2, 577, dtype=torch.bool), 'must be')):
        with pytest.raises(ValueError, match=why):
            P.as_present(bad, 2)
    for col in (0, 1):
        no_cls = full.clone()
        no_cls[1, col] = False
        with pytest.raises(ValueError, match='cls keys'):
            P.as_present(no_cls, 2)
    m, boxes = P.crop_masks(grid_regions(3), 2)
    assert tuple(m.shape) == (2, 9, 24, 24) and tuple(boxes.shape) == (2, 9, 4)
    assert bool((m.sum((2, 3)) == 64).all()) and bool(m.any(1).all()) and int(m[0, 4, 8:16, 8:16].sum()) == 64
    with pytest.raises(ValueError, match='regions'):
        P.crop_masks(torch.tensor([[0, 0, 25, 4]]), 1)


def test_to_rows():
    from vitcap_amd import patches as P

    class Tok(object):
        ids_to_tokens = {i: 'w%d' % i for i in range(200)}

        def decode(self, ids, skip_special_tokens=True):
            return ' '.join(self.ids_to_tokens[i] for i in ids if i not in (0, 101, 102))

    ids = torch.tensor([[[101, 5, 6, 102, 0], [101, 7, 102, 0, 0]]])
    topk = torch.arange(100, 200).view(1, 2, 50)
    prob = torch.linspace(0.9, 0.0, 50).repeat(1, 2, 1)
    rows = P.to_rows(ids, torch.tensor([[-0.5, -1.0]]), topk, prob, torch.tensor([[0, 0, 8, 8], [8, 16, 24, 24]]), Tok())
    assert len(rows) == 1 and len(rows[0]) == 2
    assert rows[0][0]['rect'] == [0, 0, 128, 128] and rows[0][1]['rect'] == [256, 128, 384, 384]
    assert rows[0][0]['caption'] == 'w5 w6' and abs(rows[0][1]['conf'] - np.exp(-1.0)) < 1e-9
    tags = rows[0][1]['tags']
    assert tags[0]['tag'] == 'w150' and all(t['prob'] >= 0.2 for t in tags) and len(tags) == int((prob[0, 1] >= 0.2).sum())
    with pytest.raises(ValueError, match='to_rows'):
        P.to_rows(ids[0], torch.zeros(2), topk, prob, torch.tensor([[0, 0, 8, 8]]), Tok())


def test_python_refusals_come_before_the_gpu():
    """CBS, beams (forced search), visible tags, use_graph and sampling are refused by name on a model that was never packed; so are
    bad `present` arguments and bad regions."""
    from vitcap_amd.model import ImageCaptioning
    m = ImageCaptioning(tie_weights=True).load_recipe(0).eval()
    img = torch.zeros(1, 3, 384, 384)
    ok = torch.ones(1, 24, 24, dtype=torch.bool)
    cap = torch.tensor([[101, 5, 102] + [0] * 17])
    m.refuse_patches('x')                                       # the defaults pass
    calls = {'tag_patches': lambda **kw: m.tag_patches(img, ok, **kw), 'caption_patches': lambda **kw: m.caption_patches(img, ok, **kw),
             'score_patches': lambda **kw: m.score_patches(img, cap, ok, **kw),
             'caption_crops': lambda **kw: m.caption_crops(img, torch.tensor([[0, 0, 6, 6]]), **kw),
             'caption_with_crops': lambda **kw: m.caption_with_crops(img, torch.tensor([[0, 0, 6, 6]]), **kw)}
    for name, call in calls.items():
        for kw, word in ((dict(use_cbs=True), 'use_cbs'), (dict(num_beams=3), 'num_beams'), (dict(tag_visible=5), 'tag_visible'),
                         (dict(use_graph=True), 'use_graph'), (dict(do_sample=True), 'do_sample')):
            with pytest.raises(NotImplementedError, match=word):
                call(**kw)
        assert m._packed is None, name
    with pytest.raises(ValueError, match='cls keys'):
        m.caption_patches(img, torch.zeros(1, 578, dtype=torch.bool))
    with pytest.raises(ValueError, match='present must be'):
        m.tag_patches(img, torch.ones(1, 12, 12, dtype=torch.bool))
    with pytest.raises(ValueError, match='present must be'):
        m.score_patches(img, cap, torch.ones(2, 24, 24, dtype=torch.bool))
    with pytest.raises(ValueError, match='regions'):
        m.caption_crops(img, torch.tensor([[0, 0, 0, 6]]))
    with pytest.raises(ValueError, match='regions'):
        m.caption_with_crops(img, torch.tensor([[0, 0, 30, 6]]))
    assert m._packed is None
