"""The request surface of one-pass scoring on the device: vitcap_score_req (filled by vitcap_score_req_init) through
vitcap_engine_score_req, against the positional pair vitcap_engine_score / vitcap_engine_score_text.

Everything here is bit identity: the launch sequence behind the request is that of the positional calls, and the three kinds that
add outputs (VITCAP_SCORE_MASKED with every key visible, VITCAP_SCORE_MAPS, VITCAP_SCORE_ALTS) leave the scores as the plain kind
gives them and touch no array of another kind.  raw_request is the direct caller the attention-map, alternatives and occlusion
tests share."""
import ctypes as C

import pytest
import torch

from test_hip_score_onepass import SV, S, _greedy_opts, _images, _raw_score, _variants

pytestmark = pytest.mark.gpu

PLAIN, MASKED, MAPS, ALTS = 0, 1, 2, 3      # VITCAP_SCORE_*
SENT = -7


@pytest.fixture(scope='module')
def model():
    assert torch.cuda.is_available()
    from vitcap_amd.model import ImageCaptioning
    m = ImageCaptioning(tie_weights=True, tagemb='cls').load_recipe(0).eval()
    m.pack('cuda')
    return m


def raw_request(m, img, caps, K, o, kind=PLAIN, staged=False, sws_bytes=None, sentinel=None, **fields):
    """One vitcap_engine_score_req call of `kind`, made directly: the image encoded first, or with staged the slot-0 workspace
    holds the prefill.  `fields` are further vitcap_score_req fields (tensors give their pointers): last_tok, vis_mask, maps,
    per_head, layer_mask, k, alt_ids, alt_lp, rank, entropy.  -> (rc, logprob, token_logprobs, ids, last_tok)."""
    from vitcap_amd import _lib as L
    dev = m._packed[2]
    B = caps.shape[0] // K
    ws, need = m._workspace(B, dev, 0, o)
    sneed = L.lib.vitcap_engine_score_workspace_bytes(B, K, C.byref(o))
    sws = torch.empty(max(sneed, 256), dtype=torch.uint8, device=dev)
    rows, n = caps.shape
    fill = (lambda *s, **k: torch.full(*s, fill_value=sentinel, **k)) if sentinel is not None else torch.empty
    lp = fill((rows,), dtype=torch.float32, device=dev)
    tlp = fill((rows, n), dtype=torch.float32, device=dev)
    ids = fill((rows, 1, n), dtype=torch.int64, device=dev)
    last = fill((rows,), dtype=torch.int64, device=dev)
    if fields.get('last_tok') is not None:
        fields['last_tok'] = fields['last_tok'].to(dev).contiguous()
    r = L.score_req(kind=kind, B=B, opts=o, workspace=ws, workspace_bytes=need, caps_per_image=K, caption_ids=caps.to(dev).contiguous(),
                    score_ws=sws, score_ws_bytes=sneed if sws_bytes is None else sws_bytes, out_logprobs=lp, out_token_logprobs=tlp,
                    out_ids=ids, out_last_tok=last, **fields)
    if not staged:
        r.encode, r.image, r.image_is_bf16 = 1, img.data_ptr(), int(img.dtype == torch.bfloat16)
    rc = L.lib.vitcap_engine_score_req(m._engine, C.byref(r), S())
    torch.cuda.synchronize()
    return rc, lp, tlp, ids, last


@pytest.fixture(scope='module')
def case(model):
    """2 images, 2 captions per image at max_length 12 (generate()'s own and one with a word changed), and the plain request's
    result on them, computed once and never modified."""
    o = _greedy_opts(model, max_length=12)
    img = _images(2, 56).cuda()
    ids0, _, _ = model.run(img, o, want_last=True)
    caps = _variants(ids0[:, 0].cpu(), 2)
    plain = raw_request(model, img, caps, 2, o, sentinel=SENT)
    assert plain[0] == 0 and bool(torch.isfinite(plain[1]).all())
    return o, img, caps, plain


def _same(got, want):
    return got[0] == 0 and all(torch.equal(x, y) for x, y in zip(got[1:], want[1:]))


def test_plain_request_is_the_positional_pair(model, case):
    """VITCAP_SCORE_PLAIN with encode = 1 equals vitcap_engine_score, with encode = 0 vitcap_engine_score_text: logprobs, token
    log-probs, ids and last_tok, bit for bit."""
    o, img, caps, plain = case
    assert _same(_raw_score(model, img, caps, 2, o, sentinel=SENT), plain)
    model.run(img, o, want_last=True)                                  # the prefill the staged forms read
    staged = raw_request(model, None, caps, 2, o, staged=True, sentinel=SENT)
    assert _same(staged, plain) and _same(_raw_score(model, None, caps, 2, o, staged=True, sentinel=SENT), staged)
    given = torch.tensor([2000, 2001, 2002, 2003])
    assert _same(raw_request(model, img, caps, 2, o, sentinel=SENT, last_tok=given),
                 _raw_score(model, img, caps, 2, o, last_tok=given, sentinel=SENT))


def _others(L, k=3):
    """Sentinel-filled arrays of every kind's extra outputs -> (request fields, the arrays a kind owns)."""
    dev = 'cuda'
    f = dict(maps=torch.full((4, L, 4, SV + L), float(SENT), device=dev), per_head=0, layer_mask=15, k=k,
             alt_ids=torch.full((4, L, k), SENT, dtype=torch.int32, device=dev), alt_lp=torch.full((4, L, k), float(SENT), device=dev),
             rank=torch.full((4, L), SENT, dtype=torch.int32, device=dev), entropy=torch.full((4, L), float(SENT), device=dev),
             vis_mask=torch.full((4, 19), -1, dtype=torch.int32, device=dev))
    return f, {MASKED: (), MAPS: ('maps',), ALTS: ('alt_ids', 'alt_lp', 'rank', 'entropy')}


@pytest.mark.parametrize('kind', (MASKED, MAPS, ALTS))
def test_each_kind_scores_as_plain_and_leaves_the_other_kinds_alone(model, case, kind):
    """A request of each kind with the arrays of ALL kinds handed in sentinel-filled (the mask all-visible): the score outputs are
    the plain request's bit for bit, the kind's own arrays are written, the arrays of the other kinds keep the sentinel and the
    mask is unchanged."""
    o, img, caps, plain = case
    f, owns = _others(o.max_length)
    got = raw_request(model, img, caps, 2, o, kind=kind, sentinel=SENT, **f)
    assert _same(got, plain)
    for k, mine in owns.items():
        for name in mine:
            if k == kind:
                assert bool((f[name] != SENT).any()), name
            else:
                assert bool((f[name] == SENT).all()), (kind, name)
    assert bool((f['vis_mask'] == -1).all())
