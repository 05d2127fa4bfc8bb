"""Encoder attention rollout on the device: vitcap_attn_self_maps and vitcap_rollout_step (through vitcap_amd/ops.py and
directly), vitcap_engine_encode_maps (through vitcap_amd/model.py's encoder_attention / tag_rollout / rollout_maps /
caption_with_rollout and directly).

Bounds (tests/rollout_ref.py).  vitcap_attn_self_maps against the fp64 restatement: |p - p_ref| <= 2e-4 p_ref + 1e-7, the project's
derived bound for this arithmetic.  P.V rebuilt from the per-head rows against vitcap_attn_dense_fwd: that kernel's
2e-3 + 2^-7 |want|.  vitcap_rollout_step against fp64: ((1 + gamma)^n - 1) ref + 1e-30 with gamma = gamma_580 in fp32, n = 1 for a step
and 12 for a whole path.  End to end against the reference's own `attn` (tests/golden/reference_encattn.npz) on
|p - p_ref| / (p_ref + 1e-6): twice the maximum measured on the MI355X, rounded up to one digit.  Measured figures are printed as
MEASURED lines and recorded in docs/LAB_encoder_rollout.md."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import rollout_calls as RC
import rollout_ref as R
from test_hip_score_onepass import _greedy_opts, _images

pytestmark = pytest.mark.gpu

EOS, PAD = 102, 0
NV, SV, LMAX = 577, 578, 20
SENT = 777.0
MAP_SHAPES = ((1, 16, 16), (2, 17, 17), (1, 64, 1), (3, 65, 65), (2, 577, 577), (2, 577, 1), (1, 578, 578), (1, 640, 33))      # B, S, q_rows
STEP_SHAPES = ((1, 1, 577), (2, 19, 577), (1, 40, 577), (3, 64, 33), (1, 2, 1))                                              # n_img, rows, S


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
    return dict(np.load(R.GOLDEN))


@pytest.fixture(scope='module')
def device_maps(model):
    """encoder_attention of the two seeded images, head mean and per head, computed once and shared (never modified)."""
    img = _images(2).cuda()
    mean, names = model.encoder_attention(img)
    ph, names_h = model.encoder_attention(img, per_head=True)
    assert names == list(R.BLOCK_NAMES) and names_h == names
    return img, mean, ph


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
@pytest.mark.parametrize('shape', MAP_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_self_maps_op_against_the_restatement(ops, shape, planted):
    """vitcap_attn_self_maps, both output forms: each element within 2e-4 p_ref + 1e-7 of the fp64 restatement on the same bf16 qkv;
    rows at and past q_rows exactly 0; the others sum to 1 within 1e-5; the canary around `out` untouched; the head mean the same
    bits on two runs and within 1e-6 of the mean of the per-head output."""
    B, S_, qr = shape
    qkv = R.make_qkv(B, S_, seed=5 + 3 * MAP_SHAPES.index(shape), planted=planted)
    ref = R.self_maps_ref(qkv, B, S_, qr)
    qd = qkv.cuda()
    buf, out = _framed((B, 12, S_, S_))
    ops.attn_self_maps(qd, B, S_, qr, per_head=True, out=out)
    torch.cuda.synchronize()
    assert _canary_ok(buf, out.shape)
    ph = out.cpu()
    nbad, worst = R.op_violations(ph, ref)
    print('MEASURED self maps %s %s per head: worst |p - p_ref| / (2e-4 p_ref + 1e-7) = %.3f' % (shape, 'planted' if planted else 'random', worst))
    assert nbad == 0, (nbad, worst)
    assert bool((ph[:, :, qr:] == 0).all())
    assert float((ph[:, :, :qr].double().sum(-1) - 1).abs().max()) < 1e-5
    if planted:
        assert float(ph[:, :4, :qr].max()) > 0.99          # some row holds nearly all of its mass on one key
    buf, mean = _framed((B, S_, S_))
    ops.attn_self_maps(qd, B, S_, qr, per_head=False, out=mean)
    buf2, mean2 = _framed((B, S_, S_))
    ops.attn_self_maps(qd, B, S_, qr, per_head=False, out=mean2)
    torch.cuda.synchronize()
    assert _canary_ok(buf, mean.shape) and _canary_ok(buf2, mean2.shape)
    assert torch.equal(mean, mean2)
    hm = mean.cpu()
    nbad, worst = R.op_violations(hm, ref.mean(1))
    print('MEASURED self maps %s %s head mean: worst |p - p_ref| / (2e-4 p_ref + 1e-7) = %.3f' % (shape, 'planted' if planted else 'random', worst))
    assert nbad == 0, (nbad, worst)
    assert bool((hm[:, qr:] == 0).all())
    assert float((hm[:, :qr].double().sum(-1) - 1).abs().max()) < 1e-5
    assert float((hm.double() - ph.double().mean(1)).abs().max()) < 1e-6


def test_self_maps_refusals_on_the_device(ops):
    from vitcap_amd._lib import lib
    B, S_ = 1, 33
    qd = R.make_qkv(B, S_, seed=2).cuda()
    buf, out = _framed((B, 12, S_, S_))

    def call(qkv=p(qd), o=p(out), B_=B, S__=S_, qr=S_, ph=1):
        return lib.vitcap_attn_self_maps(qkv, o, B_, S__, qr, 0.125, ph, S())

    odd = lambda t: C.c_void_p(t.data_ptr() + 2)
    for kw, name in (({'S__': 0}, b'S must'), ({'S__': 641}, b'S must'), ({'qr': 0}, b'q_rows'), ({'qr': S_ + 1}, b'q_rows'),
                     ({'ph': 2}, b'per_head'), ({'ph': -1}, b'per_head'), ({'qkv': None}, b'qkv'), ({'o': None}, b'out'),
                     ({'qkv': odd(qd)}, b'qkv'), ({'o': odd(out)}, b'out'), ({'B_': 0}, b'B must'), ({'B_': -3}, b'B must')):
        assert call(**kw) == -1, kw
        assert b'attn_self_maps' in lib.vitcap_last_error() and name in lib.vitcap_last_error(), (kw, lib.vitcap_last_error())
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out != SENT).all()) and _canary_ok(buf, out.shape)


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize('shape', ((2, 577), (1, 65)), ids=lambda s: 'x'.join(map(str, s)))
def test_self_maps_rebuild_the_dense_kernels_output(ops, shape):
    """sum_k p[k] V[k] in fp32 torch from the per-head rows against vitcap_attn_dense_fwd's output on the same qkv (that kernel
    rounds P to bf16 before its product: its own bound)."""
    B, S_ = shape
    qd = R.make_qkv(B, S_, seed=31).cuda()
    maps = ops.attn_self_maps(qd, B, S_, per_head=True)                                   # (B, 12, S, S)
    want = ops.attn_dense(qd, B, S_).float().view(B, S_, 12, 64)
    v = qd.float().view(B, S_, 3, 12, 64)[:, :, 2]                                        # (B, S, 12, 64)
    got = torch.einsum('bhqk,bkhd->bqhd', maps, v)
    err = (got - want).abs()
    bad = err > R.PV_ABS + R.PV_REL * want.abs()
    print('MEASURED self maps %s rebuilt P.V against attn_dense_fwd: max err %.3e' % (shape, float(err.max())))
    assert not bool(bad.any()), (int(bad.sum()), float(err.max()))


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize('shape', STEP_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_rollout_step_against_fp64(ops, shape):
    """vitcap_rollout_step at residual 0, 0.5 and 1 on random row-stochastic matrices (and, at S = 577, on a planted sharp one):
    each element within gamma_580 * ref + 1e-30 of fp64, row sums conserved within the same bound, residual = 1 returns v_in bit
    for bit, the canary around v_out untouched."""
    n, rows, S_ = shape
    v = R.random_rows(n, rows, S_, seed=4 + S_)
    mats = [R.random_stochastic(n, S_, seed=9 + rows)]
    if S_ == NV and n == 1:
        mats.append(R.planted_matrices(seed=7)[3])
    vd = v.cuda()
    for A in mats:
        Ad = A.cuda()
        for r in (0.0, 0.5, 1.0):
            buf, out = _framed((n, rows, S_))
            ops.rollout_step(vd, Ad, r, out=out)
            torch.cuda.synchronize()
            assert _canary_ok(buf, out.shape)
            ref = R.step_ref(v, A, r)
            nbad, worst = R.step_violations(out, ref, 1)
            print('MEASURED rollout step %s r=%.1f: worst |v - v_ref| / (gamma v_ref + 1e-30) = %.4f' % (shape, r, worst))
            assert nbad == 0, (r, nbad, worst)
            sums, want = out.double().sum(-1).cpu(), ref.sum(-1)
            assert bool(((sums - want).abs() <= R.step_rel(1) * want + S_ * R.STEP_ABS).all())
            assert float((want - v.double().sum(-1)).abs().max()) < 1e-6          # A is row-stochastic to fp32 rounding
            if r == 1.0:
                assert torch.equal(out, vd)


def test_rollout_step_refusals_on_the_device(ops):
    from vitcap_amd._lib import lib
    n, rows, S_ = 1, 3, 33
    vd, Ad = R.random_rows(n, rows, S_, seed=1).cuda(), R.random_stochastic(n, S_, seed=1).cuda()
    buf, out = _framed((n, rows, S_))

    def call(v=p(vd), A=p(Ad), o=p(out), n_=n, rows_=rows, S__=S_, r=0.5):
        return lib.vitcap_rollout_step(v, A, o, n_, rows_, S__, r, S())

    odd = lambda t: C.c_void_p(t.data_ptr() + 2)
    for kw, name in (({'v': None}, b'v_in'), ({'A': None}, b'null A'), ({'o': None}, b'v_out'), ({'v': odd(vd)}, b'aligned'),
                     ({'o': odd(out)}, b'aligned'), ({'n_': 0}, b'n_img'), ({'rows_': 0}, b'rows'), ({'rows_': 65}, b'rows'),
                     ({'S__': 0}, b'S must'), ({'S__': 641}, b'S must'), ({'r': -0.1}, b'residual'), ({'r': 1.5}, b'residual'),
                     ({'r': float('nan')}, b'residual'), ({'o': p(vd)}, b'overlaps')):
        assert call(**kw) == -1, kw
        assert b'rollout_step' in lib.vitcap_last_error() and name in lib.vitcap_last_error(), (kw, lib.vitcap_last_error())
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out != SENT).all()) and _canary_ok(buf, out.shape)


# ------------------------------------------------------------------------------------------------ 4
def test_encoder_attention_against_the_reference(model, fixture, device_maps):
    """encoder_attention() of the two seeded images against the reference's own `attn` (tests/golden/reference_encattn.npz: head-mean
    rows 0, 289, 576 of all 16 blocks, per-head row 0 of blocks.0, blocks.11, tag_blocks.3), on |p - p_ref| / (p_ref + 1e-6); the last
    tag block is compared on its row 0, the only one the device computes.  Bounds: twice the maximum measured on the MI355X, rounded
    up to one significant digit (R.E2E_BOUND_MEAN / R.E2E_BOUND_HEAD; docs/LAB_encoder_rollout.md holds the measured maxima)."""
    f = fixture
    _, mean, ph = device_maps
    assert tuple(mean.shape) == (16, 2, NV, NV) and tuple(ph.shape) == (16, 2, 12, NV, NV)
    rows = [int(r) for r in f['rows']]
    got = mean[:, :, rows].cpu().numpy()                                   # (16, 2, 3, 577)
    mx, rms = R.rel_metric(got[:15], f['mean'][:15])
    mx3, rms3 = R.rel_metric(got[15, :, 0], f['mean'][15, :, 0])
    print('MEASURED encoder_attention vs reference, head mean: max %.3e rms %.3e (tag_blocks.3 row 0: max %.3e)' % (mx, rms, mx3))
    per_block = [R.rel_metric(got[b, :, :1 if b == 15 else 3], f['mean'][b, :, :1 if b == 15 else 3])[0] for b in range(16)]
    print('MEASURED encoder_attention vs reference, head mean, per block max: %s' % ' '.join('%.2e' % x for x in per_block))
    blocks = [int(b) for b in f['per_head_blocks']]
    got_ph = ph[blocks, 0, :, 0].cpu().numpy()                             # (3, 12, 577)
    mxh, rmsh = R.rel_metric(got_ph, f['per_head'])
    print('MEASURED encoder_attention vs reference, per head: max %.3e rms %.3e' % (mxh, rmsh))
    assert max(mx, mx3) <= R.E2E_BOUND_MEAN, (mx, mx3, rms)
    assert mxh <= R.E2E_BOUND_HEAD, (mxh, rmsh)
    # the last tag block holds its cls row only; every other row of every block sums to 1; the head mean is the per-head mean
    assert bool((mean[15, :, 1:] == 0).all()) and bool((ph[15, :, :, 1:] == 0).all())
    assert float((mean[:15].double().sum(-1) - 1).abs().max()) < 1e-5 and float((mean[15, :, 0].double().sum(-1) - 1).abs().max()) < 1e-5
    assert float((mean.double() - ph.double().mean(2)).abs().max()) < 1e-6


def test_rollouts_against_the_reference(model, fixture, device_maps):
    """tag_rollout() and the rollout of the caption branch's cls (rollout_rows with w = e_1) against the fp64 rollouts the fixture
    script computed from the reference's full matrices, on |v - v_ref| / (v_ref + 1e-6).  Bound: twice the measured maximum rounded
    up to one digit (R.E2E_BOUND_ROLLOUT), which stays a factor of three below the two mutations the CPU suite measures against it
    on the fixture (test_rollout_comparison_has_teeth: image swap 0.047, column roll 0.15); no other mutation is claimed here."""
    from vitcap_amd import rollout as RO
    f = fixture
    img, mean, _ = device_maps
    grid, cls, tag_ids, tag_prob, tag_len = model.tag_rollout(img)
    assert tuple(grid.shape) == (2, 24, 24) and tuple(cls.shape) == (2,) and tuple(tag_ids.shape) == (2, 50)
    got = torch.cat([cls[:, None], grid.reshape(2, 576)], 1).cpu().numpy()
    mx, rms = R.rel_metric(got, f['tag_rollout'])
    print('MEASURED tag_rollout vs reference fp64 rollout: max %.3e rms %.3e' % (mx, rms))
    v = RO.rollout_rows(mean, R.ecls_weights(2).cuda(), 0.5)[:, 0].cpu().numpy()
    mxc, rmsc = R.rel_metric(v, f['cls_rollout'])
    print('MEASURED caption-cls rollout vs reference fp64 rollout: max %.3e rms %.3e' % (mxc, rmsc))
    assert mx <= R.E2E_BOUND_ROLLOUT and mxc <= R.E2E_BOUND_ROLLOUT, (mx, mxc)
    assert 3 * R.E2E_BOUND_ROLLOUT <= 0.047
    assert float((grid.double().sum((-1, -2)) + cls.double() - 1).abs().max()) < 1e-4
    # the tags are those of generate()'s encoder pass
    model.generate(img, want_tags=True)
    assert torch.equal(tag_ids, model.last_tags[1])


# ------------------------------------------------------------------------------------------------ 5
def _caps(fix_ids, K):
    caps = fix_ids.repeat_interleave(K, 0).clone()
    for r in range(caps.shape[0]):            # K different captions per image: cut at different lengths
        cut = LMAX - 1 - 3 * (r % K)
        caps[r, cut] = EOS
        caps[r, cut + 1:] = PAD
    return caps


def test_rollout_rows_on_planted_matrices():
    """rollout.rollout_rows on the planted matrices of the CPU suite equals the fp64 restatement within the 12-step bound (the CPU
    suite shows that every wrong walk moves that result by more than 0.5 relative)."""
    from vitcap_amd import rollout as RO
    A, w = R.planted_matrices(seed=7), R.e0_weights(1)
    got = RO.rollout_rows(A.cuda(), w.cuda(), 0.5)
    nbad, worst = R.step_violations(got, R.rollout_rows_ref(A, w, 0.5), R.PATH_STEPS)
    print('MEASURED rollout_rows planted: worst |v - v_ref| / 12-step bound = %.4f' % worst)
    assert nbad == 0, (nbad, worst)
    # more rows than one vitcap_rollout_step launch carries (64): cut into pieces, each the bits of a call of its own
    w70 = torch.rand((1, 70, SV), generator=torch.Generator().manual_seed(5)).cuda()
    got = RO.rollout_rows(A.cuda(), w70, 0.5)
    assert tuple(got.shape) == (1, 70, NV)
    assert torch.equal(got, torch.cat([RO.rollout_rows(A.cuda(), w70[:, :64].contiguous(), 0.5), RO.rollout_rows(A.cuda(), w70[:, 64:].contiguous(), 0.5)], 1))
    w2 = torch.rand((1, 5, SV), generator=torch.Generator().manual_seed(3))
    got = RO.rollout_rows(A.cuda(), w2.cuda(), 0.25)
    nbad, worst = R.step_violations(got, R.rollout_rows_ref(A, w2, 0.25), R.PATH_STEPS + 1)      # the sum at the fork rounds once more
    assert nbad == 0, (nbad, worst)


def test_tag_rollout_is_the_path_over_the_devices_matrices(model, device_maps):
    img, mean, _ = device_maps
    for r in (0.5, 0.2):
        grid, cls = model.tag_rollout(img, residual=r)[:2]
        want = R.rollout_rows_ref(mean, R.e0_weights(2), r)[:, 0]
        got = torch.cat([cls[:, None], grid.reshape(2, 576)], 1)
        nbad, worst = R.step_violations(got, want, R.PATH_STEPS)
        print('MEASURED tag_rollout r=%.1f vs fp64 path over the device matrices: worst / 12-step bound = %.4f' % (r, worst))
        assert nbad == 0, (nbad, worst)


@pytest.mark.parametrize('layers', ((0,), (0, 1, 2, 3)), ids=('l0', 'l0123'))
@pytest.mark.parametrize('K', (1, 3))
def test_rollout_maps_composition_and_scores(model, fixture, device_maps, K, layers):
    """rollout_maps equals the fp64 path recomputed from the device's own encoder_attention and attention_maps outputs within the
    12-step bound of test 3; patches.sum + cls_mass + text_mass is
    within 1e-4 of 1 on live positions, dead positions are exactly 0; the scores are score(one_pass=True)'s bit for bit."""
    import attn_maps_ref as AR
    img, mean, _ = device_maps
    caps = _caps(torch.from_numpy(np.load(os.path.join(os.path.dirname(R.GOLDEN), 'reference_attn.npz'))['ids']), K)
    lp0, tlp0 = model.score(img, caps, seqs_per_image=K, one_pass=True)
    lp0, tlp0 = lp0.clone(), tlp0.clone()
    _, _, amaps = model.attention_maps(img, caps, seqs_per_image=K, layers=layers)
    lp, tlp, grid, cls, text = model.rollout_maps(img, caps, seqs_per_image=K, layers=layers)
    assert torch.equal(lp, lp0) and torch.equal(tlp, tlp0)
    assert tuple(grid.shape) == (2 * K, LMAX, 24, 24) and tuple(cls.shape) == (2 * K, LMAX) and tuple(text.shape) == (2 * K, LMAX)
    live = AR.live_rows(caps)
    w = amaps.double().cpu()[:, :, list(layers)].mean(2)                    # (rows, L, W), not renormalised
    want = torch.stack([R.rollout_rows_ref(mean, w.view(2, K, LMAX, -1)[:, k, :, :SV], 0.5) for k in range(K)], 1).view(2 * K, LMAX, NV)
    got = torch.cat([cls[..., None], grid.reshape(2 * K, LMAX, 576)], -1).cpu()
    nbad, worst = R.step_violations(got, want, R.PATH_STEPS)
    print('MEASURED rollout_maps K=%d layers=%s vs fp64 path: worst / bound = %.4f' % (K, layers, worst))
    assert nbad == 0, (nbad, worst)
    total = got.double().sum(-1) + text.double().cpu()
    assert float((total[live] - 1).abs().max()) < 1e-4
    assert bool((got[~live] == 0).all()) and bool((text.cpu()[~live] == 0).all())
    assert float((text.double().cpu() - w[..., SV:].sum(-1)).abs().max()) < 1e-6
    lp1, tlp1 = model.score(img, caps, seqs_per_image=K, one_pass=True)
    assert torch.equal(lp1, lp0) and torch.equal(tlp1, tlp0)


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize('B', (2, 5))
def test_encode_maps_then_prefill_and_decode_is_generate(model, B):
    """vitcap_engine_encode_maps, then the staged prefill and decode calls, made directly (tests/rollout_calls.py), give generate()'s
    ids and log-probs bit for bit, under the predict loop's GEMM mode too (B = 5 is where it selects its other GEMM form);
    generate() before and after every new call is bit-identical."""
    from vitcap_amd._lib import lib
    img = _images(B).cuda()
    for gm in (0, 1):
        ids0, lp0 = model.generate(img, gemm_mode=gm)
        ids0, lp0 = ids0.clone(), lp0.clone()
        o = _greedy_opts(model, gemm_mode=gm)
        maps = torch.empty((2, B, NV, NV), dtype=torch.float32, device='cuda')
        rc, ws, need = RC.encode_maps(model, img, o, 0b1000000000000001, 0, maps)
        assert rc == 0, lib.vitcap_last_error()
        rc_p, rc_d, ids, lp = RC.prefill_and_decode(model, B, o, ws, need)
        torch.cuda.synchronize()
        assert rc_p == 0 and rc_d == 0, lib.vitcap_last_error()
        assert torch.equal(ids, ids0) and torch.equal(lp, lp0)
    cap = ids0[:, 0].clone()
    model.encoder_attention(img, blocks=[3, 'tag_blocks.1'])
    model.tag_rollout(img)
    model.rollout_maps(img, cap)
    ids_c, lp_c = model.caption_with_rollout(img, gemm_mode=1)[:2]
    assert torch.equal(ids_c, ids0) and torch.equal(lp_c, lp0)
    ids1, lp1 = model.generate(img, gemm_mode=1)
    assert torch.equal(ids1, ids0) and torch.equal(lp1, lp0)


def test_a_batch_the_plain_call_cuts_into_parts(model):
    """32 images under the predict loop's GEMM mode, where the plain encode call cuts the batch into two parts on two streams and
    runs their prefill itself.  vitcap_engine_encode_maps (one part, one stream, the prefill behind it) leaves every buffer a later
    call reads -- both hidden states, the visual tokens, the tagger's outputs, the four layers' visual K/V -- bit for bit, and the
    staged decode and caption_with_rollout return generate()'s ids and log-probs bit for bit.  (Measured: of the 1.24 GB workspace
    2 x 98 304 bytes differ, the compact cls rows of the last tag block's MLP scratch, which each part keeps at its own base and
    nothing reads afterwards; at a batch the plain call does not cut the whole workspace is compared, see
    test_block_mask_subset_writes_only_its_slots.)"""
    from vitcap_amd._lib import lib
    B = 32
    img = _images(B).cuda()
    ids0, lp0 = model.generate(img, gemm_mode=1)
    ids0, lp0 = ids0.clone(), lp0.clone()
    o = _greedy_opts(model, gemm_mode=1)
    taps = (('hidden', (B, NV, 768), torch.float32), ('tag_hidden', (B, NV, 768), torch.float32), ('vis', (B, SV, 768), torch.float32),
            ('tag_prob', (B, 50), torch.float32), ('tag_len', (B,), torch.int64)) + tuple(
                ('dqkv%d' % l, (B * SV, 2304), torch.bfloat16) for l in range(4))
    read = lambda: [model.tap(n, B, shape, dtype=dt, slot=0, opts=o) for n, shape, dt in taps]
    maps = torch.empty((1, B, NV, NV), dtype=torch.float32, device='cuda')
    rc, ws, need = RC.encode_maps(model, img, o, 1 << 7, 0, maps)
    torch.cuda.synchronize()
    assert rc == 0, lib.vitcap_last_error()
    left = read()
    assert RC.encode(model, img, o, ws, need) == 0
    torch.cuda.synchronize()
    for (name, _, _), a, b in zip(taps, left, read()):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
    rc, ws, need = RC.encode_maps(model, img, o, 1 << 7, 0, maps)
    rc_p, rc_d, ids, lp = RC.prefill_and_decode(model, B, o, ws, need)
    torch.cuda.synchronize()
    assert rc == 0 and rc_p == 0 and rc_d == 0 and torch.equal(ids, ids0) and torch.equal(lp, lp0)
    ids_c, lp_c, grid, cls, text = model.caption_with_rollout(img, gemm_mode=1)
    assert torch.equal(ids_c, ids0) and torch.equal(lp_c, lp0)
    assert float((grid.double().sum((-1, -2)) + cls.double() + text.double())[:, 1].sub(1).abs().max()) < 1e-4


def test_block_mask_subset_writes_only_its_slots(model, device_maps):
    """A block-mask subset into a sentinel-filled buffer writes its own slots only, and those hold the full call's bits, head mean
    and per head; the workspace the call leaves is the plain encode call's bit for bit."""
    from vitcap_amd._lib import lib
    img, mean, ph = device_maps
    o = _greedy_opts(model)
    sel = [2, 8, 13, 15]
    mask = sum(1 << b for b in sel)
    buf, maps = _framed((len(sel) + 1, 2, NV, NV))
    rc, ws, need = RC.encode_maps(model, img, o, mask, 0, maps[:len(sel)])
    torch.cuda.synchronize()
    assert rc == 0, lib.vitcap_last_error()
    assert _canary_ok(buf, maps.shape) and bool((maps[len(sel)] == SENT).all())
    assert torch.equal(maps[:len(sel)], mean[sel])
    left = ws[:need].clone()
    assert RC.encode(model, img, o, ws, need) == 0
    torch.cuda.synchronize()
    assert torch.equal(ws[:need], left)
    buf, maps = _framed((2, 2, 12, NV, NV))
    rc, _, _ = RC.encode_maps(model, img, o, (1 << 11) | (1 << 15), 1, maps)
    torch.cuda.synchronize()
    assert rc == 0 and _canary_ok(buf, maps.shape)
    assert torch.equal(maps, ph[[11, 15]])
    names = model.encoder_attention(img, blocks=['tag_blocks.3', 2, 'blocks.8', 13])
    assert names[1] == ['blocks.2', 'blocks.8', 'tag_blocks.1', 'tag_blocks.3'] and torch.equal(names[0], mean[sel])


def test_a_batch_larger_than_one_chunk_equals_the_per_chunk_calls(model, monkeypatch):
    from vitcap_amd import rollout as RO
    img = _images(3).cuda()
    whole = model.tag_rollout(img[:2]), model.tag_rollout(img[2:])
    att = model.encoder_attention(img[:2], blocks=[0, 15])[0], model.encoder_attention(img[2:], blocks=[0, 15])[0]
    cap = model.generate(img)[0][:, 0].clone()
    rm = model.rollout_maps(img[:2], cap[:2]), model.rollout_maps(img[2:], cap[2:])
    monkeypatch.setattr(RO, 'MAX_CALL_BYTES', RO.maps_bytes(2, 16, False))      # two images per engine call
    assert RO.images_per_call(16, False, RO.MAX_CALL_BYTES) == 2 and RO.images_per_call(2, False, RO.MAX_CALL_BYTES) == 16
    got = model.tag_rollout(img)
    for g, a, b in zip(got, *whole):
        assert torch.equal(g, torch.cat([a, b], 0))
    got = model.rollout_maps(img, cap)
    for g, a, b in zip(got, *rm):
        assert torch.equal(g, torch.cat([a, b], 0))
    # caption_with_rollout past one chunk: the captions of one generate() over the whole batch, the maps per chunk
    ids0, lp0 = model.generate(img)
    ids_c, lp_c, grid_c, cls_c, text_c = model.caption_with_rollout(img)
    assert torch.equal(ids_c, ids0) and torch.equal(lp_c, lp0)
    for g, k in ((grid_c, 2), (cls_c, 3), (text_c, 4)):
        assert torch.equal(g, torch.cat([rm[0][k], rm[1][k]], 0))
    monkeypatch.setattr(RO, 'MAX_CALL_BYTES', RO.maps_bytes(2, 2, False))
    assert torch.equal(model.encoder_attention(img, blocks=[0, 15])[0], torch.cat(att, 1))


# ------------------------------------------------------------------------------------------------ 7
def test_engine_refusals_by_name(model):
    """vitcap_engine_encode_maps refuses, by name and with nothing written: a zero mask, bits above 15, per_head outside {0, 1}, null
    or misaligned maps, maps_bytes too small, use_graph, tag_visible > 0."""
    from vitcap_amd._lib import lib
    img = _images(2).cuda()
    o = _greedy_opts(model)
    buf, maps = _framed((1, 2, NV, NV))
    ws, need = model._workspace(2, img.device, 'refusals', o)
    ws.fill_(7)

    def call(o_=o, mask=1, ph=0, m=maps, nbytes=None):
        return RC.encode_maps(model, img, o_, mask, ph, m, maps_bytes=nbytes, ws=ws)[0]

    og, ot = _greedy_opts(model), _greedy_opts(model)
    og.use_graph, ot.tag_visible = 1, 3
    for kw, name in ((dict(mask=0), b'block_mask'), (dict(mask=1 << 16), b'block_mask'), (dict(ph=2), b'per_head'), (dict(ph=-1), b'per_head'),
                     (dict(nbytes=maps.numel() * 4 - 1), b'maps_bytes'), (dict(mask=3), b'maps_bytes'), (dict(o_=og), b'use_graph'),
                     (dict(o_=ot), b'tag_visible')):
        assert call(**kw) == -1, kw
        assert b'encode_maps' in lib.vitcap_last_error() and name in lib.vitcap_last_error(), (kw, lib.vitcap_last_error())
    B = 2
    assert lib.vitcap_engine_encode_maps(model._engine, p(img), 0, B, C.byref(o), p(ws), need, 1, 0, None, maps.numel() * 4, S()) == -1
    assert b'maps is null' in lib.vitcap_last_error()
    assert lib.vitcap_engine_encode_maps(model._engine, p(img), 0, B, C.byref(o), p(ws), need, 1, 0, C.c_void_p(maps.data_ptr() + 2),
                                         maps.numel() * 4, S()) == -1
    assert b'aligned' in lib.vitcap_last_error()
    torch.cuda.synchronize()
    assert bool((buf == SENT).all()) and bool((ws == 7).all())
    # the Python surface refuses the same by the option's name, before the GPU is touched
    for kw, name in ((dict(use_cbs=True), 'use_cbs'), (dict(num_beams=3), 'num_beams'), (dict(tag_visible=2), 'tag_visible'),
                     (dict(do_sample=True), 'do_sample'), (dict(use_graph=True), 'use_graph')):
        with pytest.raises(NotImplementedError, match=name):
            model.tag_rollout(img, **kw)


@pytest.mark.parametrize('n_img', (2, 5))
def test_pipeline_writes_the_rollout_tsv(model, tmp_path, monkeypatch, n_img):
    """ensure_predict with `rollout: true` on 2 images, and on 5 (from 4 images on the predict loop's GEMM mode picks another GEMM
    form than the default): the .rollout.tsv rows decode (vitcap_amd.rollout.from_rows) and equal tag_rollout's map and
    caption_with_rollout's maps of the live words rounded the same way; the prediction TSV is byte-identical to a run without the
    key; a prediction file without its rollout file is written again; the combinations the key is not built for are refused."""
    import json
    from oracle import vitcap_oracle as O
    from vitcap_amd.pipeline import CaptionUniPipeline
    from vitcap_amd.rollout import from_rows
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
    with_ro = run('ro', rollout=True)
    assert open(plain, 'rb').read() == open(with_ro, 'rb').read()
    assert not os.path.exists(plain[:-4] + '.rollout.tsv')
    ro = with_ro[:-4] + '.rollout.tsv'
    assert with_ro.endswith('.predict.tsv') and os.path.isfile(ro) and os.path.isfile(ro[:-4] + '.lineidx')
    again = run('plain', force=False, rollout=True)          # predictions exist, their rollout file does not: both are written
    assert again == plain and open(plain[:-4] + '.rollout.tsv', 'rb').read() == open(ro, 'rb').read()
    ids, lp, grid, cls, text, tag_same, tag_cls = model.caption_with_rollout(img.cuda(), want_tag=True, gemm_mode=1)      # the predict loop's GEMM mode
    tag, tag_cls0 = model.tag_rollout(img.cuda(), gemm_mode=1)[:2]
    assert torch.equal(tag_same, tag) and torch.equal(tag_cls, tag_cls0)          # the tag map of the caption's own encoder pass
    want, want_tag = grid.cpu().numpy().astype(np.float16), tag.cpu().numpy().astype(np.float16)
    rows = [l.rstrip('\n').split('\t') for l in open(ro)]
    assert [r[0] for r in rows] == keys
    for b, (key, js) in enumerate(rows):
        tokens, tag_map, word_maps = from_rows(json.loads(js))
        ends = [t for t in range(1, LMAX) if int(ids[b, 0, t]) == EOS]
        n = ends[0] if ends else LMAX - 1
        assert tokens == [toks[int(t)] for t in ids[b, 0, 1:n + 1]] and word_maps.shape == (n, 24, 24)
        assert np.array_equal(tag_map, want_tag[b]) and np.array_equal(word_maps, want[b, 1:n + 1])
        assert 0.9 < float(tag_map.astype(np.float64).sum()) <= 1.001
    for kw, name in ((dict(num_beams=2), 'num_beams'), (dict(caption_prefix='w5 w6'), 'caption_prefix'), (dict(attention_maps=True), 'attention_maps'),
                     (dict(alternatives=3), 'alternatives'), (dict(occlusion=4), 'occlusion'), (dict(regions=2), 'regions'),
                     (dict(crops=2), 'crops'), (dict(tag_visible=2), 'tag_visible')):
        with pytest.raises(NotImplementedError, match=name):
            run('bad', rollout=True, **kw)
