"""One-pass caption scoring: what is decided on the host, without a GPU.

score(one_pass=True) refuses what the one-pass path does not run before it touches the image (the `image` handed in here is a
host tensor that no engine call could take), and the engine entry points refuse the same options, null arguments and a short score
workspace on an engine without weights, with pointers that are never followed."""
import ctypes as C

import pytest
import torch

BOS, EOS, PAD = 101, 102, 0


@pytest.fixture(scope='module')
def L():
    from vitcap_amd import _lib
    return _lib


@pytest.fixture(scope='module')
def model():
    from vitcap_amd.model import ImageCaptioning
    return ImageCaptioning(tie_weights=True, tagemb='cls')


def _caps(rows, max_len=20):
    c = torch.full((rows, max_len), 2000, dtype=torch.int64)
    c[:, 0] = BOS
    c[:, -1] = EOS
    return c


def test_score_one_pass_refuses_before_touching_the_image(model):
    img = torch.zeros(2, 1)          # never a valid image: every refusal below comes first
    for over, name in (({'num_beams': 2}, 'num_beams'), ({'use_cbs': True}, 'use_cbs'), ({'repetition_penalty': 1.3}, 'repetition_penalty'),
                       ({'tag_visible': 5}, 'tag_visible'), ({'do_sample': True}, 'do_sample')):
        with pytest.raises(NotImplementedError, match=name):
            model.score(img, _caps(2), one_pass=True, **over)
    with pytest.raises(NotImplementedError, match='seqs_per_image'):
        model.score(img, _caps(66), seqs_per_image=33, one_pass=True)
    bad = _caps(2)
    bad[1, 0] = 2000
    with pytest.raises(ValueError, match=r'\[CLS\]'):
        model.score(img, bad, one_pass=True)
    with pytest.raises(ValueError, match='vocabulary'):
        model.score(img, _caps(2) + 40000, one_pass=True)
    with pytest.raises(ValueError):
        model.score(img, _caps(3), one_pass=True)          # 3 rows for 2 images x 1 caption
    # 32 captions per image, a second EOS id and max_length 40 pass the host checks
    o, cap, lt = model._score_inputs(2, _caps(64, 40), 32, [5] * 64, {'eos_token_ids': [EOS, 1012], 'max_length': 40})
    assert tuple(cap.shape) == (64, 40) and tuple(lt.shape) == (64,) and o.max_length == 40 and o.eos_extra[0] == 1012
    with pytest.raises(RuntimeError, match='no encoded images'):
        model.score_encoded(_caps(2))


def test_stepwise_score_keeps_its_cap(model, L):
    """one_pass=False is today's path: nine captions per image are refused by the option check, as before."""
    with pytest.raises(L.VitcapError, match='seqs_per_image must be 1..8'):
        model.score(torch.zeros(1, 1), _caps(9), seqs_per_image=9)


def test_engine_score_entry_points_refuse_without_a_device(L):
    lib = L.lib
    h = C.c_void_p()
    assert lib.vitcap_engine_create(C.byref(h)) == 0 and h.value
    buf = (C.c_char * 1024)()
    a = C.c_void_p((C.addressof(buf) + 255) & ~255)
    big = 1 << 40

    def text(o, K=1, ids=a, sws=a, sws_bytes=big, lp=a, out_ids=a):
        return lib.vitcap_engine_score_text(h, 1, C.byref(o) if o is not None else None, a, 512, K, ids, None, sws, sws_bytes, lp, None,
                                            out_ids, None, None)

    def whole(o, K=1, ids=a, sws=a, sws_bytes=big, lp=a, out_ids=a):
        return lib.vitcap_engine_score(h, a, 0, 1, C.byref(o) if o is not None else None, a, 512, K, ids, None, sws, sws_bytes, lp, None,
                                       out_ids, None, None)

    sp = L.SampleParams(1, 1.0, 0, 1.0, 0)
    refused = ((L.gen_opts(num_beams=2), b'num_beams'),
               (L.gen_opts(use_cbs=1, cbs_states=8, fsm=4096, num_constraints=4096), b'use_cbs'),
               (L.gen_opts(tag_visible=5), b'tag_visible'),
               (L.gen_opts(sampling=sp), b'do_sample'),
               (L.gen_opts(repetition_penalty=1.3), b'repetition_penalty'))
    for fn in (text, whole):
        for o, name in refused:
            assert fn(o) == -1 and name in lib.vitcap_last_error(), name
            assert lib.vitcap_engine_score_workspace_bytes(1, 1, C.byref(o)) == 0
        for K in (0, 33):
            assert fn(None, K=K) == -1 and b'caps_per_image' in lib.vitcap_last_error()
        assert fn(None, ids=None) == -1 and b'null' in lib.vitcap_last_error()
        assert fn(None, lp=None) == -1 and fn(None, out_ids=None) == -1 and fn(None, sws=None) == -1
        assert fn(L.gen_opts(max_length=41)) == -1 and b'max_length' in lib.vitcap_last_error()
        need = lib.vitcap_engine_score_workspace_bytes(1, 1, None)
        assert fn(None, sws_bytes=need - 1) == -3 and b'score workspace' in lib.vitcap_last_error()
        assert fn(None, sws_bytes=need) == -4                          # everything checked: the unbound engine is reported
    lib.vitcap_engine_destroy(h)


def test_score_workspace_size(L):
    """The table of csrc/engine_layout.h: grows with the captions, the logits chunk is bounded at 2048 rows."""
    lib = L.lib
    w = lambda B, K, **kw: lib.vitcap_engine_score_workspace_bytes(B, K, C.byref(L.gen_opts(**kw)))
    assert w(1, 1) % 256 == 0 and w(2, 3) > w(2, 2) > w(1, 2)
    assert 0.6e9 < w(64, 5) < 0.7e9 and 2.4e9 < w(64, 32) < 2.6e9       # the sizes the header states
    assert w(64, 32) < 2048 * 19 * 30592 * 4                           # far below the unchunked logits alone
    assert w(1, 1, max_length=40) > w(1, 1) and w(1, 0) == 0 and w(0, 1) == 0
    # the existing workspace does not know about it
    o = L.gen_opts()
    assert lib.vitcap_engine_workspace_bytes(2, C.byref(o)) == lib.vitcap_engine_workspace_bytes(2, None)


def test_op_launchers_refuse_bad_shapes(L):
    lib = L.lib
    buf = (C.c_char * 1024)()
    a = C.c_void_p((C.addressof(buf) + 255) & ~255)
    for n_img, K, S, ml, name in ((1, 1, 577, 20, b'S_vis'), (1, 1, 578, 41, b'max_len'), (1, 1, 578, 1, b'max_len'),
                                  (1, 33, 578, 20, b'caps_per_image'), (1, 0, 578, 20, b'caps_per_image')):
        assert lib.vitcap_attn_text_grid(a, a, a, a, n_img, K, S, ml, 0.125, None) == -1
        assert b'attn_text_grid' in lib.vitcap_last_error() and name in lib.vitcap_last_error()
    assert lib.vitcap_attn_text_grid(None, a, a, a, 1, 1, 578, 20, 0.125, None) == -1
    args = lambda rows0, n, L_: (a, 30592, 30522, a, None, rows0, n, 2, L_, EOS, None, PAD, None, None, a, a, None, a, None)
    assert lib.vitcap_score_rows(*args(0, 39, 20)) == -1 and b'score_rows' in lib.vitcap_last_error()      # 2 x 19 = 38 rows
    assert lib.vitcap_score_rows(*args(0, 1, 41)) == -1 and lib.vitcap_score_rows(*args(-1, 1, 20)) == -1
