"""Occlusion maps of given captions on the device: vitcap_attn_text_grid_masked, vitcap_engine_score_req with kind
VITCAP_SCORE_MASKED (directly and through vitcap_amd/model.py's score_masked / score_masked_encoded / occlusion_maps /
visual_gain / caption_with_occlusion) and the pipeline's `occlusion: window`.

Bounds.  Attention: |err| <= 2e-3 + 2^-7 |want| against the rounding emulation, the bound of tests/test_hip_score_onepass.py test 1.
End to end against the oracle's forward as written with the hidden columns zeroed in the joint mask: 4e-2 per token and 1e-2 per
sequence, the bounds of that file's test 5.  Everything else is bit identity.  Measured figures are printed as MEASURED lines and
recorded in docs/LAB_occlusion.md."""
import ctypes as C
import json
import os

import pytest
import torch

import occlusion_ref as R
from test_hip_score_onepass import (BOS, EOS, LMAX, PAD, SEQ_TOL, SV, TOK_TOL, S, _bf, _close, _greedy_opts, _images, _rand, _raw_score,
                                    _variants, p)
from test_hip_score_request import MASKED, raw_request

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    from vitcap_amd import ops as o
    return o


@pytest.fixture(scope='module')
def model():
    assert torch.cuda.is_available()
    from vitcap_amd.model import ImageCaptioning
    m = ImageCaptioning(tie_weights=True, tagemb='cls').load_recipe(0).eval()
    m.pack('cuda')
    return m


def _pack(visible, high_bits=False):
    """bool (NC, 578) -> device int32 (NC, 19); high_bits: the ignored bits 578..607 set."""
    from vitcap_amd.occlusion import pack_visible
    w = pack_visible(visible)
    if high_bits:
        w[:, 18] |= torch.tensor(-4, dtype=torch.int32)          # word 18: bits 2..31 = keys 578..607
    return w.cuda().contiguous()


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize('K,L', [(1, 20), (3, 8), (2, 2), (2, 40), (9, 20), (32, 20)])
def test_all_ones_mask_is_the_unmasked_kernel(ops, K, L):
    """vitcap_attn_text_grid_masked with every key visible equals vitcap_attn_text_grid bit for bit, with the ignored bits 578..607
    set or clear.  B = 2."""
    n_img, R_ = 2, 2 * L - 1
    NC = n_img * K
    vis = _bf(_rand((n_img, SV, 2304), 240 + K, 2.0)).reshape(n_img * SV, 2304).cuda().contiguous()
    text = _bf(_rand((NC, R_, 2304), 241 + L, 2.0)).reshape(NC * R_, 2304).cuda().contiguous()
    want = ops.attn_text_grid(text, vis, n_img, K, SV, L)
    ones = torch.ones(NC, SV, dtype=torch.bool)
    for high in (False, True):
        got = ops.attn_text_grid_masked(text, vis, _pack(ones, high), n_img, K, SV, L)
        torch.cuda.synchronize()
        assert torch.equal(got, want), 'K=%d L=%d high bits %s' % (K, L, high)
    assert bool(torch.isfinite(want.float()).all())


# ------------------------------------------------------------------------------------------------ 2
def test_masks_against_the_emulation(ops):
    """2 images x 9 captions (the second group of a workgroup's 8 starts inside an image), max_len 20, a different mask per caption
    and per image: random 50 %, all hidden, only key 0, only key 577, keys 16..31 hidden, single bits 15, 16, 31, 32, 575, 576, 577
    hidden (occlusion_ref.MASK_KINDS in turn).  Within 2e-3 + 2^-7 |want| of the rounding emulation on every row but token row
    L - 1; the canary behind `out` intact."""
    n_img, K, L = 2, 9, 20
    R_, NC = 2 * L - 1, n_img * K
    vis = _bf(_rand((n_img, SV, 2304), 250, 2.0)).reshape(n_img * SV, 2304)
    text = _bf(_rand((NC, R_, 2304), 251, 2.0)).reshape(NC * R_, 2304)
    visible = R.masks_by_kind(NC, 252)
    assert len(set(R.MASK_KINDS)) == 12 and NC >= 12 and not torch.equal(visible[:K], visible[K:])
    buf = torch.full((NC * R_ + 64, 768), 7.0, dtype=torch.bfloat16, device='cuda')
    got = ops.attn_text_grid_masked(text.cuda().contiguous(), vis.cuda().contiguous(), _pack(visible), n_img, K, SV, L, out=buf)
    torch.cuda.synchronize()
    assert bool((buf[NC * R_:] == 7.0).all()), 'canary behind out overwritten'
    assert bool(torch.isfinite(got[:NC * R_].float()).all())
    want = R.masked_grid_ref(text, vis, visible, n_img, K, L)
    keep = [r for r in range(R_) if r != L - 1]
    got = got[:NC * R_].view(NC, R_, 768).cpu()
    for c in range(NC):
        worst = _close(got[c:c + 1, keep], want[c:c + 1, keep], 'masked text-grid attention, caption %d (%s)' % (c, R.MASK_KINDS[c % 12]))
        print('MEASURED attn_text_grid_masked caption %2d %-10s: max |err| %.3e' % (c, R.MASK_KINDS[c % 12], worst))
    # the masks matter: against the unmasked emulation the all-hidden caption is far outside the bound
    plain = R.masked_grid_ref(text, vis, torch.ones_like(visible), n_img, K, L)
    assert R.violations(got[1:2, keep], plain[1:2, keep])[0] > 0


# ------------------------------------------------------------------------------------------------ 3
def test_planted_keys(ops):
    """Planted inputs (occlusion_ref.planted_inputs), 2 images x 9 captions, max_len 8: hiding the planted keys moves exactly the
    planted slices -- the same set as in the restatement -- to the reference's values; each mutated reference misses the bound."""
    n_img, K, L = 2, 9, 8
    R_, NC = 2 * L - 1, n_img * K
    x, v, visible, planted = R.planted_inputs(n_img, K, L, 33)
    xd, vd = x.cuda().contiguous(), v.cuda().contiguous()
    plain = ops.attn_text_grid(xd, vd, n_img, K, SV, L).view(NC, R_, 768).cpu()
    got = ops.attn_text_grid_masked(xd, vd, _pack(visible), n_img, K, SV, L).view(NC, R_, 768).cpu()
    keep = [r for r in range(R_) if r != L - 1]
    want = R.masked_grid_ref(x, v, visible, n_img, K, L)
    worst = _close(got[:, keep], want[:, keep], 'masked text-grid attention on planted inputs')
    moved, inside, outside = R.moved(got, plain, L)
    print('MEASURED planted: max |err| %.3e; %d slices moved, smallest move %.3f, largest elsewhere %.3e' % (worst, len(moved), inside, outside))
    assert moved == planted and len(planted) == NC * 4
    for mutate in R.MUTATIONS:
        bad, far = R.violations(got[:, keep], R.masked_grid_ref(x, v, visible, n_img, K, L, mutate=mutate)[:, keep])
        print('MEASURED planted, mutation %-16s: %d elements outside the bound, max |d| %.3f' % (mutate, bad, far))
        assert bad > 0, mutate


# ------------------------------------------------------------------------------------------------ 4
def test_attn_text_grid_masked_refusals(ops):
    """A null mask, a mask at an address that is not 4-byte aligned, S_vis = 577, max_len = 41 and 33 captions are refused by name with
    `out` untouched."""
    from vitcap_amd._lib import lib
    a = torch.zeros((4096, 2304), dtype=torch.bfloat16, device='cuda')
    vt = torch.zeros((1, 12, 64, 608), dtype=torch.bfloat16, device='cuda')
    out = torch.full((4096, 768), 7.0, dtype=torch.bfloat16, device='cuda')
    mask = torch.full((33 * 19 + 1,), -1, dtype=torch.int32, device='cuda')
    odd = C.c_void_p(mask.data_ptr() + 2)
    for m, K, Sv, L, name in ((None, 1, 578, 20, b'vis_mask is null'), (odd, 1, 578, 20, b'vis_mask is not 4-byte aligned'),
                              (p(mask), 1, 577, 20, b'S_vis'), (p(mask), 1, 578, 41, b'max_len'), (p(mask), 33, 578, 20, b'caps_per_image')):
        assert lib.vitcap_attn_text_grid_masked(p(a), p(a), p(vt), m, p(out), 1, K, Sv, L, 0.125, S()) == -1
        assert b'attn_text_grid_masked' in lib.vitcap_last_error() and name in lib.vitcap_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ 5
def test_score_masked_all_ones_is_score_one_pass(model):
    """score_masked with everything visible equals score(one_pass=True) bit for bit -- logprob, token_logprobs and ids -- in both
    shapes of `visible`, and differs once keys are hidden."""
    img = _images(2, 56).cuda()
    ids0, _ = model.generate(img)
    caps = _variants(ids0[:, 0].cpu(), 3)
    want = model.score(img, caps, seqs_per_image=3, return_ids=True, one_pass=True)
    for visible in (torch.ones(6, 578, dtype=torch.bool), torch.ones(6, 578, dtype=torch.uint8), torch.ones(6, 24, 24, dtype=torch.bool)):
        got = model.score_masked(img, caps, visible, seqs_per_image=3, return_ids=True)
        assert all(torch.equal(x, y) for x, y in zip(got, want))
    half = torch.ones(6, 24, 24, dtype=torch.bool)
    half[:, :, :12] = False
    lp_h, tlp_h = model.score_masked(img, caps, half, seqs_per_image=3)
    assert not torch.equal(lp_h, want[0]) and bool(torch.isfinite(tlp_h).all())
    enc = model.score_masked_encoded(caps, half, seqs_per_image=3)
    assert torch.equal(enc[0], lp_h) and torch.equal(enc[1], tlp_h)


def test_engine_score_masked_staged_and_grouping(model):
    """A VITCAP_SCORE_MASKED request with encode = 1 equals prefill + the same request with encode = 0 bit for bit; 12 variants per image equal three
    K = 4 calls bit for bit; generate() afterwards is unchanged and so are the K / V columns of dqkv0..3."""
    img = _images(2, 57).cuda()
    ids0, lp0 = model.generate(img)
    o = _greedy_opts(model)
    caps = _variants(ids0[:, 0].cpu(), 12)
    caps[5, 8], caps[5, 9:] = EOS, PAD
    visible = torch.rand(24, 578, generator=torch.Generator().manual_seed(3)) < 0.7
    visible[0] = True
    visible[13] = False
    mask = _pack(visible)
    whole = raw_request(model, img, caps, 12, o, kind=MASKED, vis_mask=mask)
    assert whole[0] == 0 and bool(torch.isfinite(whole[1]).all())
    model.run(img, o, want_last=True)
    taps = [model.tap('dqkv%d' % l, 2, (2 * SV, 2304), dtype=torch.bfloat16, opts=o) for l in range(4)]
    assert float(taps[0][:, 768:].float().abs().max()) > 0
    staged = raw_request(model, None, caps, 12, o, kind=MASKED, vis_mask=mask, staged=True)
    assert staged[0] == 0 and all(torch.equal(x, y) for x, y in zip(staged[1:], whole[1:]))
    c3, m3 = caps.view(2, 3, 4, LMAX), mask.view(2, 3, 4, 19)
    for j in range(3):
        part = raw_request(model, None, c3[:, j].reshape(8, LMAX), 4, o, kind=MASKED, vis_mask=m3[:, j].reshape(8, 19).contiguous(), staged=True)
        sel = (torch.arange(2)[:, None] * 12 + j * 4 + torch.arange(4)[None]).reshape(-1)
        assert part[0] == 0
        for x, y in zip(part[1:], whole[1:]):
            assert torch.equal(x, y[sel.to(y.device)]), 'K = 12 against K = 4, part %d' % j
    for l in range(4):
        assert torch.equal(model.tap('dqkv%d' % l, 2, (2 * SV, 2304), dtype=torch.bfloat16, opts=o)[:, 768:], taps[l][:, 768:])
    plain = _raw_score(model, None, caps, 12, o, staged=True)       # the unmasked pair on the same prefill: caption 0 sees everything
    assert plain[0] == 0 and torch.equal(plain[2][0], whole[2][0]) and not torch.equal(plain[2][13], whole[2][13])
    ids1, lp1 = model.generate(img)
    assert torch.equal(ids1, ids0) and torch.equal(lp1, lp0)


def test_engine_score_masked_refusals_on_the_device(model):
    """Every refused option returns VITCAP_EINVAL with its name and leaves the outputs' sentinel, so does a null mask; a score
    workspace one byte short returns VITCAP_EWORKSPACE (as test_engine_score_refusals_on_the_device)."""
    from vitcap_amd import _lib as L
    lib = L.lib
    img = _images(1, 59).cuda()
    caps = torch.full((1, LMAX), 2000, dtype=torch.int64)
    caps[:, 0], caps[:, -1] = BOS, EOS
    model.generate(img)
    mask = torch.full((33, 19), -1, dtype=torch.int32, device='cuda')
    fsm = torch.zeros(8, dtype=torch.uint8, device='cuda')
    refused = ((L.gen_opts(num_beams=2), b'num_beams'),
               (L.gen_opts(use_cbs=1, cbs_states=8, fsm=fsm.data_ptr(), num_constraints=fsm.data_ptr()), b'use_cbs'),
               (L.gen_opts(tag_visible=5), b'tag_visible'),
               (L.gen_opts(sampling=L.SampleParams(1, 1.0, 0, 1.0, 0)), b'do_sample'),
               (L.gen_opts(repetition_penalty=1.3), b'repetition_penalty'))
    o = _greedy_opts(model)

    def untouched(r):
        return all(bool((x == -7).all()) for x in r[1:])

    for staged in (False, True):
        for bad, name in refused:
            r = raw_request(model, img, caps, 1, bad, kind=MASKED, vis_mask=mask, staged=staged, sentinel=-7)
            assert r[0] == -1 and name in lib.vitcap_last_error() and untouched(r), name
        r = raw_request(model, img, caps.repeat(33, 1), 33, o, kind=MASKED, vis_mask=mask, staged=staged, sentinel=-7)
        assert r[0] == -1 and b'caps_per_image' in lib.vitcap_last_error() and untouched(r)
        r = raw_request(model, img, caps, 1, o, kind=MASKED, vis_mask=None, staged=staged, sentinel=-7)
        assert r[0] == -1 and b'vis_mask is null' in lib.vitcap_last_error() and untouched(r)
        need = lib.vitcap_engine_score_workspace_bytes(1, 1, C.byref(o))
        r = raw_request(model, img, caps, 1, o, kind=MASKED, vis_mask=mask, staged=staged, sws_bytes=need - 1, sentinel=-7)
        assert r[0] == -3 and untouched(r)
    r = raw_request(model, img, caps, 1, o, kind=MASKED, vis_mask=mask, sentinel=-7)       # and the accepted call writes every output
    assert r[0] == 0 and not untouched(r) and bool(torch.isfinite(r[1]).all())


# ------------------------------------------------------------------------------------------------ 6
def test_against_the_reference_semantics(model, sd_t):
    """One golden image, max_length 8, the device's own greedy caption; the oracle's forward as written, looped over cur_len with the
    hidden visual columns zeroed in the caption rows of the joint mask (occlusion_ref.token_logprobs_as_written; the encoder is
    computed once).  Two masks: the left 12 patch columns hidden, all 578 keys hidden.  Per token within 4e-2, per sequence within
    1e-2.  The all-hidden result differs from the unmasked one by more than the per-token bound on at least one token -- on the
    device, and in the oracle alone."""
    L = 8
    img = _images(1, 1234)
    o = _greedy_opts(model, max_length=L)
    ids0, _, last = model.run(img.cuda(), o, want_last=True)
    ids = ids0[:, 0].cpu()
    scored = ids.clone()
    if not bool((ids[0, 1:-1] == EOS).any()):
        scored[0, -1] = last.cpu()[0]                      # the token the last position is scored on
    left = torch.ones(1, 24, 24, dtype=torch.bool)
    left[:, :, :12] = False
    from vitcap_amd.occlusion import as_visible
    masks = {'all visible': torch.ones(1, 578, dtype=torch.bool), 'left half hidden': as_visible(left, 1),
             'all hidden': torch.zeros(1, 578, dtype=torch.bool)}
    want, got, enc = {}, {}, None
    with torch.no_grad():
        for name, vis in masks.items():
            lp_w, tlp_w, enc = R.token_logprobs_as_written(sd_t, img, scored, vis, L, enc=enc)
            want[name] = (lp_w, tlp_w)
            lp_g, tlp_g, ids_g = model.score_masked(img.cuda(), ids, vis, return_ids=True, last_tok=last, max_length=L)
            assert torch.equal(ids_g.cpu(), ids0.cpu())
            got[name] = (lp_g.cpu(), tlp_g.cpu())
    for name in masks:
        d_tok = float((got[name][1] - want[name][1]).abs().max())
        d_seq = float((got[name][0] - want[name][0]).abs().max())
        print('MEASURED %-16s: max |token_lp - oracle| %.3e, |sequence - oracle| %.3e' % (name, d_tok, d_seq))
    gap_oracle = float((want['all hidden'][1] - want['all visible'][1]).abs().max())
    gap_device = float((got['all hidden'][1] - got['all visible'][1]).abs().max())
    gap_left = float((want['left half hidden'][1] - want['all visible'][1]).abs().max())
    print('MEASURED all hidden against all visible, largest per-token gap: oracle %.3f, device %.3f; left half hidden, oracle %.3f'
          % (gap_oracle, gap_device, gap_left))
    assert gap_oracle > TOK_TOL and gap_device > TOK_TOL
    for name in masks:
        assert float((got[name][1] - want[name][1]).abs().max()) <= TOK_TOL, name
        assert float((got[name][0] - want[name][0]).abs().max()) <= SEQ_TOL, name


# ------------------------------------------------------------------------------------------------ 7
def test_occlusion_maps(model):
    """window 4: 36 windows + the baseline = 37 variants per image, more than one scoring pass holds.  Equal, bit for bit, to one
    score_masked_encoded call per variant; shape (2, L, 6, 6); zero at position 0 and behind the end.  At window 24 with keep_cls
    off it is visual_gain.  caption_with_occlusion's ids are generate()'s."""
    from vitcap_amd.occlusion import window_masks
    img = _images(2, 56).cuda()
    ids0, lp0 = model.generate(img)
    caps = ids0[:, 0].cpu().clone()
    caps[1, 6], caps[1, 7:] = EOS, PAD
    lp, tlp, drop = model.occlusion_maps(img, caps, window=4)
    assert tuple(lp.shape) == (2,) and tuple(tlp.shape) == (2, LMAX) and tuple(drop.shape) == (2, LMAX, 6, 6)
    assert bool((drop[:, 0] == 0).all()) and bool((drop[1, 7:] == 0).all()) and bool(torch.isfinite(drop).all())
    assert float(drop[0, 1:].abs().max()) > 0 and float(drop[1, 1:7].abs().max()) > 0
    base = model.score(img, caps, one_pass=True)
    assert torch.equal(base[0], lp) and torch.equal(base[1], tlp)
    masks = window_masks(4)
    for g in (0, 7, 30, 31, 35):                                       # either side of the 32-variant pass limit
        _, tlp_g = model.score_masked_encoded(caps, masks[g:g + 1].repeat(2, 1))
        assert torch.equal(drop[:, :, g // 6, g % 6], tlp - tlp_g), 'window %d' % g
    for keep_only in (False, True):
        lp_e, tlp_e, drop_e = model.occlusion_maps_encoded(caps, window=8, stride=4, keep_only=keep_only)
        assert tuple(drop_e.shape) == (2, LMAX, 5, 5) and torch.equal(tlp_e, tlp)
        m = window_masks(8, 4, keep_only=keep_only)
        _, tlp_g = model.score_masked_encoded(caps, m[13:14].repeat(2, 1))
        assert torch.equal(drop_e[:, :, 2, 3], tlp - tlp_g)
    gain = model.visual_gain(img, caps)
    _, _, whole = model.occlusion_maps(img, caps, window=24, keep_cls=False)
    assert tuple(whole.shape) == (2, LMAX, 1, 1) and torch.equal(whole[:, :, 0, 0], gain)
    gain3 = model.visual_gain(img, _variants(caps, 3), seqs_per_image=3)
    assert tuple(gain3.shape) == (6, LMAX) and torch.equal(gain3[0::3], gain)
    print('MEASURED occlusion_maps window 4: largest drop %.3f, most negative %.3f; visual_gain: largest %.3f'
          % (float(drop.max()), float(drop.min()), float(gain.max())))
    ids_c, lp_c, drop_c = model.caption_with_occlusion(img, window=8)
    assert torch.equal(ids_c, ids0) and torch.equal(lp_c, lp0) and tuple(drop_c.shape) == (2, LMAX, 3, 3)
    assert bool((drop_c[:, 0] == 0).all()) and float(drop_c.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 8
class _Tok:
    def __init__(self, toks):
        self.ids_to_tokens = toks


@pytest.mark.parametrize('n_img', (2, 5))
def test_pipeline_writes_the_occlusion_tsv(model, tmp_path, monkeypatch, n_img):
    """ensure_predict with `occlusion: 8` on 2 images and on 5: the .occ.tsv rows are to_rows of caption_with_occlusion; the prediction
    TSV is byte-identical to a run without the key; every combination the occlusion maps are not built for is refused by name."""
    from oracle import vitcap_oracle as O
    from vitcap_amd.occlusion import to_rows
    from vitcap_amd.pipeline import CaptionUniPipeline
    monkeypatch.chdir(tmp_path)
    enc = tmp_path / 'enc'
    enc.mkdir()
    toks = ['[PAD]'] + ['w%d' % i for i in range(1, 30522)]
    toks[100], toks[101], toks[102], toks[103] = '[UNK]', '[CLS]', '[SEP]', '[MASK]'
    (enc / 'vocab.txt').write_text('\n'.join(toks) + '\n')
    img = _images(n_img)
    keys = ['k%d' % i for i in range(n_img)]

    def batch():
        input_ids, am = O.test_text_inputs(n_img)
        return {'image': img.clone(), 'key': list(keys), 'input_ids': input_ids, 'attention_mask': am,
                'token_type_ids': torch.zeros(n_img, 70, dtype=torch.long)}

    def run(name, force=True, **kw):
        pl = CaptionUniPipeline(full_expid='E', init_recipe_seed=0, text_encoder_type=str(enc), tagemb='cls', force_predict=force,
                                test_batches=[batch()], model_file=str(tmp_path / (name + '.pt')), **kw)
        return pl.ensure_predict()

    plain = run('plain')
    with_occ = run('occ', occlusion=8)
    assert open(plain, 'rb').read() == open(with_occ, 'rb').read()
    assert not os.path.exists(plain[:-4] + '.occ.tsv')
    occ = with_occ[:-4] + '.occ.tsv'
    assert with_occ.endswith('.predict.tsv') and os.path.isfile(occ) and os.path.isfile(occ[:-4] + '.lineidx')
    ids, lp, drop = model.caption_with_occlusion(img.cuda(), window=8, gemm_mode=1)      # the predict loop's GEMM mode
    want = to_rows(ids.cpu(), drop.cpu(), _Tok(toks))
    rows = [l.rstrip('\n').split('\t') for l in open(occ)]
    assert [r[0] for r in rows] == keys
    for b, (key, js) in enumerate(rows):
        recs = json.loads(js)
        assert recs == want[b] and len(recs) > 0
        assert all(len(rec['drop']) == 3 and len(rec['drop'][0]) == 3 for rec in recs)
    for kw, name in (({'num_beams': 2}, 'num_beams'), ({'use_cbs': True}, 'use_cbs'), ({'caption_prefix': 'w5 w6'}, 'caption_prefix'),
                     ({'tag_visible': 5}, 'tag_visible'), ({'attention_maps': True}, 'attention_maps'), ({'alternatives': 3}, 'alternatives')):
        with pytest.raises(NotImplementedError, match=name):
            run('refused', occlusion=8, **kw)
