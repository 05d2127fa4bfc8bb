"""Attention maps of given captions on the device: vitcap_attn_probe_maps (through ops.attn_probe_maps and directly),
vitcap_engine_score_req with kind VITCAP_SCORE_MAPS (through vitcap_amd/model.py's attention_maps / attention_maps_encoded /
caption_with_maps and directly).

Bounds.  The op against the fp64 restatement of the row definition (tests/attn_maps_ref.py): |p - p_ref| <= 2e-4 p_ref + 1e-7,
derived there.  The op against vitcap_attn_text_grid (P.V rebuilt from the per-head rows): that kernel's 2e-3 + 2^-7 |want|.  End to
end against the reference's own attention_probs (tests/golden/reference_attn.npz) on |p - p_ref| / (p_ref + 1e-6): measured on the
MI355X max 2.24e-3 (head mean) and 8.69e-3 (per head); bounds twice that, rounded up to one digit: 5e-3 and 2e-2.  Measured figures are
printed as MEASURED lines and recorded in docs/LAB_attention_maps.md."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import attn_maps_ref as R
from test_hip_score_onepass import _greedy_opts, _images
from test_hip_score_request import MAPS, raw_request

pytestmark = pytest.mark.gpu

EOS, PAD, BOS = 102, 0, 101
SV, LMAX = 578, 20
SENT = 777.0
SHAPES = ((2, 1, 20), (1, 3, 8), (1, 2, 40), (1, 2, 2), (1, 9, 20))       # n_images, caps_per_image, max_len
# R.captions ends caption c % 4 == 0 at position 1 and c % 4 == 1 at L // 2, so at two captions no row behind L // 2 is live in
# SHAPES.  These two shapes run with every position live (all three query tiles and all three token-key blocks at L = 40).
ALL_LIVE = ((2, 1, 40), (2, 1, 8))


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


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


@pytest.fixture(scope='module')
def fixture():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_attn.npz')))


_CASES = {}


def _case(shape, planted):
    """Inputs, captions and the fp64 restatement of one shape, computed once and shared (never modified)."""
    key = (shape, planted)
    if key not in _CASES:
        n, K, L = shape
        idx = (SHAPES + ALL_LIVE).index(shape)
        q, v = R.make_inputs(n, K, L, seed=11 + 7 * idx, planted=planted)
        ids = R.captions(n * K, L, seed=3 + idx)
        if shape in ALL_LIVE:
            ids[ids == EOS] = 2000
            ids[ids == PAD] = 2001
        _CASES[key] = (q, v, ids, R.probe_maps_ref(q, v, ids, n, K, L))
    return _CASES[key]


def _framed(shape, pad=1024):
    """A sentinel-filled buffer with `shape` in its middle -> (whole buffer, the view)."""
    n = int(np.prod(shape))
    buf = torch.full((pad + n + pad,), SENT, dtype=torch.float32, device='cuda')
    return buf, buf[pad:pad + n].view(shape)


def _canary_ok(buf, shape, pad=1024):
    n = int(np.prod(shape))
    return bool((buf[:pad] == SENT).all()) and bool((buf[pad + n:] == SENT).all())


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize('planted', (False, True), ids=('random', 'planted'))
@pytest.mark.parametrize('shape', SHAPES + ALL_LIVE, ids=lambda s: 'x'.join(map(str, s)))
def test_probe_maps_op_against_the_restatement(ops, shape, planted):
    """vitcap_attn_probe_maps, both output forms, on every layer slot in turn: each element within 2e-4 p_ref + 1e-7 of the fp64
    restatement; dead rows and dead columns exactly 0; live rows sum to 1 within 1e-5; the other layers' slices and the canary
    around `out` untouched; the head mean the same bits on two runs and within 1e-6 of the mean of the per-head rows."""
    n, K, L = shape
    W, NC = SV + L, n * K
    q, v, ids, ref = _case(shape, planted)
    qd, vd, idd = q.cuda(), v.cuda(), ids.cuda()
    live = R.live_rows(ids)
    assert shape not in ALL_LIVE or bool(live[:, 1:].all())
    layer = (SHAPES + ALL_LIVE).index(shape) % 4
    # per head
    buf, out = _framed((NC, L, 4, 12, W))
    ops.attn_probe_maps(qd, vd, idd, n, K, max_len=L, per_head=True, layer=layer, out=out)
    torch.cuda.synchronize()
    assert _canary_ok(buf, out.shape)
    others = [l for l in range(4) if l != layer]
    assert bool((out[:, :, others] == SENT).all())
    ph = out[:, :, layer].cpu()
    nbad, worst = R.op_violations(ph, ref)
    print('MEASURED probe maps %s %s per head: worst |p - p_ref| / (2e-4 p_ref + 1e-7) = %.3f' % (shape, 'planted' if planted else 'random', worst))
    assert nbad == 0, (nbad, worst)
    assert bool((ph[~live] == 0).all())
    for t in range(1, L):
        assert bool((ph[:, t, :, SV + t + 1:] == 0).all())
    sums = ph.double().sum(-1)
    assert float((sums[live] - 1).abs().max()) < 1e-5
    # head mean, twice
    buf, mean = _framed((NC, L, 4, W))
    ops.attn_probe_maps(qd, vd, idd, n, K, max_len=L, per_head=False, layer=layer, out=mean)
    buf2, mean2 = _framed((NC, L, 4, W))
    ops.attn_probe_maps(qd, vd, idd, n, K, max_len=L, per_head=False, layer=layer, out=mean2)
    torch.cuda.synchronize()
    assert _canary_ok(buf, mean.shape) and bool((mean[:, :, others] == SENT).all())
    assert torch.equal(mean, mean2)
    hm = mean[:, :, layer].cpu()
    nbad, worst = R.op_violations(hm, R.head_mean(ref))
    print('MEASURED probe maps %s %s head mean: worst |p - p_ref| / (2e-4 p_ref + 1e-7) = %.3f' % (shape, 'planted' if planted else 'random', worst))
    assert nbad == 0, (nbad, worst)
    assert bool((hm[~live] == 0).all())
    for t in range(1, L):
        assert bool((hm[:, t, SV + t + 1:] == 0).all())
    assert float((hm.double().sum(-1)[live] - 1).abs().max()) < 1e-5
    assert float((hm.double() - ph.double().mean(-2)).abs().max()) < 1e-6


def test_probe_maps_second_eos_id(ops):
    """eos_extra ends a caption like eos does."""
    n, K, L = 1, 3, 8
    q, v, ids, _ = _case((1, 3, 8), False)
    ids = ids.clone()
    ids[2] = torch.tensor([BOS, 2000, 2001, 1012, 2002, 2003, 2004, EOS])
    ref = R.probe_maps_ref(q, v, ids, n, K, L, eos_extra=(1012,))
    out = ops.attn_probe_maps(q.cuda(), v.cuda(), ids.cuda(), n, K, max_len=L, per_head=True, layer=0, eos_extra=(1012,))
    assert R.op_violations(out[:, :, 0].cpu(), ref)[0] == 0
    assert bool((out[2, 4:, 0] == 0).all()) and bool((out[2, 3, 0].sum(-1) > 0.99).all())


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize('shape', ((1, 3, 8), (1, 9, 20)) + ALL_LIVE, ids=lambda s: 'x'.join(map(str, s)))
def test_probe_maps_rebuild_the_grid_kernels_output(ops, shape):
    """sum_k p[k] V[k] over the visual, token and self V rows, in fp32 torch from the per-head rows, against vitcap_attn_text_grid's
    output on the probe rows of the same buffers (that kernel rounds P to bf16 before its product: its own bound).  Every
    position is live, so at (2,1,40) all 39 probe rows -- three query tiles, three token-key blocks -- are compared."""
    n, K, L = shape
    R_, NC = 2 * L - 1, n * K
    q, v, ids, _ = _case(shape, False)
    ids = ids.clone()
    ids[ids == EOS] = 2000                 # every position live
    qd, vd = q.cuda(), v.cuda()
    maps = ops.attn_probe_maps(qd, vd, ids.cuda(), n, K, max_len=L, per_head=True, layer=2)[:, :, 2]      # (NC, L, 12, W)
    grid = ops.attn_text_grid(qd, vd, n, K, max_len=L).view(NC, R_, 12, 64)[:, L:].float()                # probe rows (NC, L-1, 12, 64)
    x = qd.float().view(NC, R_, 2304)
    v_vis = vd.float().view(n, SV, 2304)[:, :, 1536:].reshape(n, SV, 12, 64).repeat_interleave(K, 0)      # (NC, 578, 12, 64)
    v_tok = x[:, :L, 1536:].reshape(NC, L, 12, 64)
    v_self = x[:, L:, 1536:].reshape(NC, L - 1, 12, 64)
    pm = maps[:, 1:]                                                                                     # (NC, L-1, 12, W)
    got = torch.einsum('cjhk,ckhd->cjhd', pm[..., :SV], v_vis)
    tok = pm[..., SV:].clone()                                                                           # (NC, L-1, 12, L): tokens, then self at t
    t_idx = torch.arange(1, L, device='cuda').view(1, L - 1, 1, 1).expand(NC, L - 1, 12, 1)
    p_self = tok.gather(-1, t_idx)
    tok.scatter_(-1, t_idx, 0.0)
    got = got + torch.einsum('cjhk,ckhd->cjhd', tok, v_tok) + p_self * v_self
    err = (got - grid).abs()
    bad = err > 2e-3 + 2 ** -7 * grid.abs()
    print('MEASURED probe maps %s rebuilt P.V against attn_text_grid: max err %.3e' % (shape, float(err.max())))
    assert not bool(bad.any()), (int(bad.sum()), float(err.max()))


# ------------------------------------------------------------------------------------------------ 3
def test_probe_maps_refusals_on_the_device(ops):
    from vitcap_amd._lib import lib
    n, K, L = 1, 2, 8
    q, v = R.make_inputs(n, K, L, seed=2)
    qd, vd, idd = q.cuda(), v.cuda(), R.captions(n * K, L, seed=2).cuda()
    buf, out = _framed((n * K, L, 4, 12, SV + L))

    def call(qkv=p(qd), vis=p(vd), ids=p(idd), o=p(out), n_=n, K_=K, S_=SV, L_=L, ph=1):
        return lib.vitcap_attn_probe_maps(qkv, vis, ids, o, n_, K_, S_, L_, ph, EOS, None, 0.125, S())

    odd = lambda t: C.c_void_p(t.data_ptr() + 2)
    for kw, name in (({'S_': 577}, b'S_vis'), ({'S_': 579}, b'S_vis'), ({'L_': 1}, b'max_len'), ({'L_': 41}, b'max_len'),
                     ({'K_': 0}, b'caps_per_image'), ({'K_': 33}, b'caps_per_image'), ({'ph': 2}, b'per_head'), ({'ph': -1}, b'per_head'),
                     ({'qkv': None}, b'qkv_text'), ({'vis': None}, b'vis_qkv'), ({'ids': None}, b'caption_ids'), ({'o': None}, b'out'),
                     ({'qkv': odd(qd)}, b'aligned'), ({'vis': odd(vd)}, b'aligned'), ({'ids': odd(idd)}, b'misaligned'),
                     ({'o': odd(out)}, b'misaligned'), ({'n_': 0}, b'n_images')):
        assert call(**kw) == -1, kw
        assert b'attn_probe_maps' in lib.vitcap_last_error() and name in lib.vitcap_last_error(), (kw, lib.vitcap_last_error())
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out[:, :, 0] != SENT).all()) and _canary_ok(buf, out.shape)


# ------------------------------------------------------------------------------------------------ engine helpers
# ------------------------------------------------------------------------------------------------ 4
def test_attention_maps_against_the_reference(model, fixture):
    """attention_maps() on the reference's own greedy captions of the two seeded images against the reference's attention_probs
    (tests/golden/reference_attn.npz: [MASK] rows of steps 1, 5, 10, 19, all four layers), on |p - p_ref| / (p_ref + 1e-6).
    Measured on the MI355X: head mean max 2.243e-3 rms 4.84e-4, per head max 8.691e-3 rms 1.785e-3.  Bounds: twice the measured
    maximum, rounded up to one significant digit -- 5e-3 (head mean) and 2e-2 (per head)."""
    f = fixture
    img = _images(2).cuda()
    caps = torch.from_numpy(f['ids'])
    lp, tlp, mean = model.attention_maps(img, caps)
    _, _, ph = model.attention_maps(img, caps, per_head=True)
    assert tuple(mean.shape) == (2, LMAX, 4, SV + LMAX) and tuple(ph.shape) == (2, LMAX, 4, 12, SV + LMAX)
    steps = [int(t) for t in f['steps']]
    got = mean[:, steps].cpu().numpy()                                 # (2, 4 steps, 4 layers, W)
    mx, rms = R.rel_metric(got, f['mean'])
    print('MEASURED attention_maps vs reference, head mean: max %.3e rms %.3e' % (mx, rms))
    psteps, players = [int(t) for t in f['per_head_steps']], [int(l) for l in f['per_head_layers']]
    got_ph = ph[0][psteps][:, players].cpu().numpy()                   # (2 steps, 2 layers, 12, W)
    mxh, rmsh = R.rel_metric(got_ph, f['per_head'])
    print('MEASURED attention_maps vs reference, per head: max %.3e rms %.3e' % (mxh, rmsh))
    assert mx <= R.E2E_BOUND_MEAN, (mx, rms)
    assert mxh <= R.E2E_BOUND_HEAD, (mxh, rmsh)
    assert abs(float(lp[0]) - float(f['logprobs'][0, 0])) < 1e-2
    # position 0 is zeros; both captions run to the last column, so every other row is live and sums to 1
    assert bool((mean[:, 0] == 0).all()) and float((mean[:, 1:].double().sum(-1) - 1).abs().max()) < 1e-5
    assert float((mean.double() - ph.double().mean(-2)).abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize('K', (1, 3))
def test_scores_are_those_of_score_one_pass(model, fixture, K):
    """attention_maps() returns the logprobs / token_logprobs of score(one_pass=True) bit for bit, and a score() call after it
    gives the same bits as before it."""
    img = _images(2).cuda()
    base = torch.from_numpy(fixture['ids'])
    caps = base.repeat_interleave(K, 0).clone()
    for r in range(caps.shape[0]):            # K different captions per image: cut at different lengths
        cut = LMAX - 1 - 3 * (r % K)
        caps[r, cut] = EOS
        caps[r, cut + 1:] = PAD
    lp0, tlp0 = model.score(img, caps, seqs_per_image=K, one_pass=True)
    lp0, tlp0 = lp0.clone(), tlp0.clone()
    for per_head, layers in ((False, (0, 1, 2, 3)), (True, (3,))):
        lp, tlp, maps = model.attention_maps(img, caps, seqs_per_image=K, per_head=per_head, layers=layers)
        assert torch.equal(lp, lp0) and torch.equal(tlp, tlp0)
        live = R.live_rows(caps).cuda()
        assert bool((maps[~live] == 0).all())
        sel = maps[:, :, list(layers)]
        assert float((sel[live].double().sum(-1) - 1).abs().max()) < 1e-5
    lp1, tlp1 = model.score(img, caps, seqs_per_image=K, one_pass=True)
    assert torch.equal(lp1, lp0) and torch.equal(tlp1, tlp0)


def test_generate_is_unchanged_by_an_attention_maps_call(model, fixture):
    img = _images(2).cuda()
    ids0, lp0 = model.generate(img)
    ids0, lp0 = ids0.clone(), lp0.clone()
    model.attention_maps(img, torch.from_numpy(fixture['ids']), per_head=True)
    ids1, lp1 = model.generate(img)
    assert torch.equal(ids0, ids1) and torch.equal(lp0, lp1)


def test_unselected_layers_are_left_untouched(model, fixture):
    """VITCAP_SCORE_MAPS requests (encode = 1 and 0) directly, layer_mask 0b0101 into a sentinel-filled array: layers 1 and 3
    and the canary around the array keep the sentinel, layers 0 and 2 are those of a full call; a zero mask, a null array and a bad
    per_head are refused with nothing written."""
    img = _images(2).cuda()
    caps = torch.from_numpy(fixture['ids'])
    o = _greedy_opts(model)
    _, _, full = model.attention_maps(img, caps)
    for staged in (False, True):
        buf, maps = _framed((2, LMAX, 4, SV + LMAX))
        rc, lp, tlp, ids, _ = raw_request(model, img, caps, 1, o, kind=MAPS, staged=staged, maps=maps, per_head=0, layer_mask=0b0101)
        assert rc == 0
        assert _canary_ok(buf, maps.shape) and bool((maps[:, :, [1, 3]] == SENT).all())
        assert torch.equal(maps[:, :, [0, 2]], full[:, :, [0, 2]])
        assert torch.equal(ids[:, 0].cpu(), caps)
    from vitcap_amd._lib import lib
    buf, maps = _framed((2, LMAX, 4, SV + LMAX))
    for kw, name in ((dict(per_head=0, mask=0), b'layer_mask'), (dict(per_head=0, mask=16), b'layer_mask'), (dict(per_head=2, mask=15), b'per_head')):
        assert raw_request(model, img, caps, 1, o, kind=MAPS, maps=maps, per_head=kw['per_head'], layer_mask=kw['mask'])[0] == -1
        assert name in lib.vitcap_last_error()
    assert raw_request(model, img, caps, 1, o, kind=MAPS, maps=None, per_head=0, layer_mask=15)[0] == -1 and b'maps' in lib.vitcap_last_error()
    assert bool((buf == SENT).all())


# ------------------------------------------------------------------------------------------------ 6
def test_staged_forms(model, fixture):
    """attention_maps_encoded after generate() gives the bits of the whole call; caption_with_maps returns generate()'s ids and the
    maps of its own caption; 12 captions per image equal three calls of 4."""
    img = _images(2).cuda()
    ids, lp = model.generate(img)
    caps = ids[:, 0].clone()
    lp_e, tlp_e, maps_e = model.attention_maps_encoded(caps)
    maps_e = maps_e.clone()
    lp_w, tlp_w, maps_w = model.attention_maps(img, caps)
    assert torch.equal(maps_e, maps_w) and torch.equal(lp_e, lp_w) and torch.equal(tlp_e, tlp_w)
    ids_c, lp_c, maps_c = model.caption_with_maps(img)
    assert torch.equal(ids_c, ids) and torch.equal(lp_c, lp)
    assert torch.equal(maps_c, maps_w)            # the maps do not depend on last_tok: it only picks the scored token
    _, _, maps_c3 = model.caption_with_maps(img, per_head=True, layers=(3,))
    assert bool((maps_c3[:, :, :3] == 0).all())
    assert float((maps_c3[:, :, 3].double().mean(-2) - maps_w[:, :, 3].double()).abs().max()) < 1e-6
    # 12 captions per image = three calls of 4
    base = caps.cpu()
    caps12 = base.repeat_interleave(12, 0).clone()
    g = torch.Generator().manual_seed(9)
    for r in range(caps12.shape[0]):
        n_live = 2 + (r * 5) % (LMAX - 2)
        caps12[r, 1:n_live] = torch.randint(1000, 30000, (n_live - 1,), generator=g)
        caps12[r, n_live] = EOS
        caps12[r, n_live + 1:] = PAD
    lp12, tlp12, maps12 = model.attention_maps(img, caps12, seqs_per_image=12)
    v12 = maps12.view(2, 12, LMAX, 4, SV + LMAX)
    c12 = caps12.view(2, 12, LMAX)
    for part in range(3):
        sub = c12[:, 4 * part:4 * part + 4].reshape(8, LMAX)
        lp4, tlp4, maps4 = model.attention_maps(img, sub, seqs_per_image=4)
        assert torch.equal(maps4.view(2, 4, LMAX, 4, SV + LMAX), v12[:, 4 * part:4 * part + 4])
        assert torch.equal(lp4.view(2, 4), lp12.view(2, 12)[:, 4 * part:4 * part + 4])


@pytest.mark.parametrize('L', (8, 40))
def test_other_max_lengths(model, L):
    """max_length 8 and 40 at B = 2: width 578 + L, dead rows and columns zero, rows sum to 1, the head mean is the per-head rows'
    mean, the staged call equals the whole call."""
    img = _images(2).cuda()
    ids, lp = model.generate(img, max_length=L)
    caps = ids[:, 0].clone()
    lp_w, tlp_w, mean = model.attention_maps(img, caps, max_length=L)
    _, _, ph = model.attention_maps(img, caps, per_head=True, max_length=L)
    _, _, mean_e = model.attention_maps_encoded(caps, max_length=L)
    W = SV + L
    assert tuple(mean.shape) == (2, L, 4, W) and tuple(ph.shape) == (2, L, 4, 12, W)
    assert torch.equal(mean, mean_e)
    live = R.live_rows(caps.cpu()).cuda()
    assert bool((mean[~live] == 0).all()) and bool((ph[~live] == 0).all())
    assert float((mean[live].double().sum(-1) - 1).abs().max()) < 1e-5
    for t in range(1, L):
        assert bool((ph[:, t, :, :, SV + t + 1:] == 0).all())
    assert float((mean.double() - ph.double().mean(-2)).abs().max()) < 1e-6
    lp_s, tlp_s = model.score(img, caps, one_pass=True, max_length=L)
    assert torch.equal(lp_s, lp_w) and torch.equal(tlp_s, tlp_w)


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize('n_img', (2, 5))
def test_pipeline_writes_the_attention_tsv(model, tmp_path, monkeypatch, n_img):
    """ensure_predict with `attention_maps: true` on 2 images, and on 5 (from 4 images on the predict loop's GEMM mode picks another
    GEMM form than the default): the .attn.tsv rows decode to (n_tokens, 24, 24) float16 and equal caption_with_maps' last-layer
    patch block rounded the same way; the prediction TSV is byte-identical to a run without the key; a prediction file without
    its attention file is written again; beam search or a caption prefix together with the key is refused."""
    import base64
    import json
    from oracle import vitcap_oracle as O
    from vitcap_amd.attnmaps import patch_grid
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
    with_maps = run('maps', attention_maps=True)
    assert open(plain, 'rb').read() == open(with_maps, 'rb').read()
    assert not os.path.exists(plain[:-4] + '.attn.tsv')
    attn = with_maps[:-4] + '.attn.tsv'
    assert with_maps.endswith('.predict.tsv') and os.path.isfile(attn) and os.path.isfile(attn[:-4] + '.lineidx')
    again = run('plain', force=False, attention_maps=True)          # predictions exist, their attention file does not: both are written
    assert again == plain and os.path.isfile(plain[:-4] + '.attn.tsv')
    assert open(plain, 'rb').read() == open(with_maps, 'rb').read() and open(plain[:-4] + '.attn.tsv', 'rb').read() == open(attn, 'rb').read()
    ids, lp, maps = model.caption_with_maps(img.cuda(), gemm_mode=1)          # the predict loop's GEMM mode
    want = patch_grid(maps[:, :, 3]).to(torch.float16).cpu().numpy()
    rows = [l.rstrip('\n').split('\t') for l in open(attn)]
    assert [r[0] for r in rows] == keys
    for b, (key, js) in enumerate(rows):
        rec = json.loads(js)
        n = len(rec['tokens'])
        ends = [t for t in range(1, LMAX) if int(ids[b, 0, t]) == EOS]
        assert rec['layer'] == 3 and rec['dtype'] == 'float16' and rec['shape'] == [n, 24, 24] and n == ends[0]
        assert rec['tokens'] == [toks[int(t)] for t in ids[b, 0, 1:n + 1]]
        got = np.frombuffer(base64.b64decode(rec['data']), dtype=np.float16).reshape(rec['shape'])
        assert np.array_equal(got, want[b, 1:n + 1])
        assert 0.9 < float(got.astype(np.float64).sum((-1, -2)).min()) <= 1.0          # the patches hold nearly all of a row's mass
    with pytest.raises(NotImplementedError, match='attention_maps'):
        run('beam', attention_maps=True, num_beams=2)
    with pytest.raises(NotImplementedError, match='caption_prefix'):
        run('prefix', attention_maps=True, caption_prefix='w5 w6')
