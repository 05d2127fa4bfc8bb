"""Forced tokens in the decode loop, the parts that need no GPU: the host packing (vitcap_amd/forced.py) with every refusal, the
refusals of beam search / CBS at the Python surface and at the two engine entry points (checked before any GPU work), and the
forced "sampler" the GPU tests use as their expectation, pinned against the oracle's own greedy run."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(REPO, 'vitcap_amd', 'libvitcap_hip.so')):
        g.build()
    from vitcap_amd import _lib
    return _lib


def forced_sampler(forced, temperature=1.0):
    """sampler(logits, t) for oracle.vitcap_oracle.greedy_incremental that takes forced[:, t] where it is >= 0 and the argmax
    elsewhere; log-prob = log_softmax(logits / temperature) at the token taken (unfiltered).  The GPU tests' expectation."""
    forced = torch.as_tensor(forced)

    def sampler(logits, t):
        x = logits / temperature if temperature != 1.0 else logits
        free = x.argmax(-1)
        f = forced[:, t]
        tok = torch.where(f >= 0, f, free)
        lp = torch.log_softmax(x, -1).gather(1, tok[:, None])[:, 0]
        top2 = x.topk(2, -1).values
        return tok, lp, top2[:, 0] - top2[:, 1]
    return sampler


def test_pack_forced_prefix(L):
    from vitcap_amd.forced import pack_forced
    f, sf = pack_forced(prefix_ids=[[7, 8, 9], [5, -1, -1]], rows=2, max_length=6)
    assert sf == 0 and f.dtype == torch.int64 and tuple(f.shape) == (2, 6)
    assert f.tolist() == [[-1, 7, 8, 9, -1, -1], [-1, 5, -1, -1, -1, -1]]
    f, sf = pack_forced(prefix_ids=torch.full((3, 0), -1), rows=3, max_length=4)            # an empty prefix: everything free
    assert sf == 0 and bool((f == -1).all())
    f, _ = pack_forced(prefix_ids=np.arange(19)[None] + 1000, rows=1, max_length=20)        # P = max_length - 1 is the longest
    assert f[0, 1:].tolist() == list(range(1000, 1019)) and f[0, 0] == -1


def test_pack_forced_caption(L):
    from vitcap_amd.forced import pack_forced
    cap = torch.tensor([[101, 5, 6, 102, 0, 0], [101, 5, 6, 7, 8, 102], [101, 9, 102, 102, 7, 0], [101, 5, 6, 7, 8, 9]])
    f, sf = pack_forced(caption_ids=cap, rows=4, max_length=6)
    assert sf == 1
    # row 1: the [SEP] in the last column of a caption that had not ended is the max-length rule's, not a choice: left free
    assert f.tolist() == [[-1, 5, 6, 102, -1, -1], [-1, 5, 6, 7, 8, -1], [-1, 9, 102, -1, -1, -1], [-1, 5, 6, 7, 8, 9]]
    f, _ = pack_forced(caption_ids=cap, rows=4, max_length=6, last_tok=[11, 12, 13, 14])     # ... or the token the caller knows
    assert f[:, -1].tolist() == [-1, 12, -1, 9]
    with pytest.raises(ValueError, match='last_tok'):
        pack_forced(caption_ids=cap, rows=4, max_length=6, last_tok=[1, 2, 3])


@pytest.mark.parametrize('kw,msg', [
    (dict(), 'exactly one'),
    (dict(prefix_ids=[[1]], caption_ids=[[101, 102]]), 'exactly one'),
    (dict(prefix_ids=[[1, 2, 3, 4]]), 'leaves 3'),                        # P > max_length - 1
    (dict(prefix_ids=[[30522]]), 'vocabulary'),
    (dict(prefix_ids=[[-2]]), 'vocabulary'),
    (dict(prefix_ids=[[-1, 5]]), 'follows a -1'),
    (dict(prefix_ids=[1, 2]), r'must be \(1, n\)'),
    (dict(prefix_ids=[[1], [2]]), r'must be \(1, n\)'),                   # rows
    (dict(prefix_ids=[[1.5]]), 'integer'),
    (dict(caption_ids=[[101, 5, 102]]), r'must be \(1, 4\)'),
    (dict(caption_ids=[[100, 5, 102, 0]]), 'CLS'),
    (dict(caption_ids=[[101, 5, 30522, 0]]), 'vocabulary'),
    (dict(caption_ids=[[101, -1, 102, 0]]), 'vocabulary'),
    (dict(caption_ids=[[101, 5, 102, 0], [101, 5, 102, 0]]), r'must be \(1, n\)'),
])
def test_pack_forced_refusals(L, kw, msg):
    from vitcap_amd.forced import pack_forced
    with pytest.raises(ValueError, match=msg):
        pack_forced(rows=1, max_length=4, **kw)


def test_pack_forced_refuses_bad_sizes(L):
    from vitcap_amd.forced import pack_forced
    for rows, ml in ((0, 20), (None, 20), (1, 1), (1, 41)):
        with pytest.raises(ValueError, match='rows >= 1'):
            pack_forced(prefix_ids=[[1]], rows=rows, max_length=ml)


def test_python_surface_refuses_forced_beam_and_cbs(L):
    """A prefix with num_beams > 1 or use_cbs raises NotImplementedError before anything touches a GPU; it is never ignored."""
    from vitcap_amd.model import ImageCaptioning
    m = ImageCaptioning(tie_weights=True).eval()
    img = torch.zeros(1, 3, 384, 384)
    for bad in ({'num_beams': 2}, {'use_cbs': True}):
        keep = dict(m.test_extra_input)
        m.test_extra_input.update(bad)
        with pytest.raises(NotImplementedError, match='forced tokens under beam search'):
            m({'image': img, 'key': [0], 'prefix_ids': torch.tensor([[2023]])})
        m.test_extra_input['prefix_ids'] = torch.tensor([[2023]])           # the same through test_extra_input
        with pytest.raises(NotImplementedError, match='forced tokens under beam search'):
            m({'image': img, 'key': [0]})
        m.test_extra_input = keep
    with pytest.raises(NotImplementedError):
        ImageCaptioning.refuse_forced_search(5, False)
    ImageCaptioning.refuse_forced_search(1, False)
    # run() itself refuses too, before it looks at the image: options with beams and a forced array
    with pytest.raises(NotImplementedError, match='forced tokens under beam search'):
        m.run(img, m.gen_options(num_beams=2), forced=torch.full((1, 20), -1))
    with pytest.raises(NotImplementedError, match='forced tokens under beam search'):
        m.run(img, m.gen_options(num_beams=2), want_token_logprobs=True)


def test_engine_entry_points_refuse_forced_beam_and_cbs(L):
    """vitcap_engine_decode_forced / vitcap_engine_generate_forced: VITCAP_EINVAL with a message for num_beams = 2 and for CBS, on an
    engine without weights and with pointers that are never followed -- the check comes before any GPU work.  Without forced ids
    and per-token output the same options are not refused by this check (the unbound engine is then reported, VITCAP_ESTATE)."""
    lib = L.lib
    h = C.c_void_p()
    assert lib.vitcap_engine_create(C.byref(h)) == 0 and h.value
    buf = (C.c_char * 1024)()
    a = C.c_void_p((C.addressof(buf) + 255) & ~255)
    beams = L.gen_opts(num_beams=2)
    cbs = L.gen_opts(use_cbs=1, cbs_states=8, num_beams=2, fsm=4096, num_constraints=4096)
    for o in (beams, cbs):
        for forced, tlp in ((a, None), (None, a), (a, a)):
            assert lib.vitcap_engine_decode_forced(h, 1, C.byref(o), a, 512, forced, 1, a, a, tlp, None, None) == -1
            assert b'num_beams == 1' in lib.vitcap_last_error() and b'forced' in lib.vitcap_last_error()
            assert lib.vitcap_engine_generate_forced(h, a, 0, 1, C.byref(o), a, 512, forced, 0, a, a, tlp, None, None, None) == -1
            assert b'num_beams == 1' in lib.vitcap_last_error()
    assert lib.vitcap_engine_decode_forced(h, 1, C.byref(beams), a, 512, None, 0, a, a, None, None, None) == -4
    assert lib.vitcap_engine_generate_forced(h, a, 0, 1, C.byref(beams), a, 512, None, 0, a, a, None, None, None, None) == -4
    # score_forced is 0 or 1; broken options are reported as such
    assert lib.vitcap_engine_decode_forced(h, 1, None, a, 512, a, 2, a, a, None, None, None) == -1
    assert b'score_forced' in lib.vitcap_last_error()
    assert lib.vitcap_engine_decode_forced(h, 1, C.byref(L.gen_opts(num_beams=9)), a, 512, a, 1, a, a, None, None, None) == -1
    assert b'num_beams must be 1..8' in lib.vitcap_last_error()
    # the op-level launchers validate before they launch
    assert lib.vitcap_greedy_step_forced(a, 30592, 30522, a, a, a, a, a, None, None, 1, 1, 20, 102, 0, a, 2, None, None) == -1
    assert lib.vitcap_greedy_select_embed_forced(a, 956, None, 0, 0, a, a, a, a, a, None, 1, 19, 20, 102, 0, 103, None, None, None, None,
                                                 None, 1e-12, None, None, a, 1, None, None) == -1
    assert b'logits' in lib.vitcap_last_error()
    lib.vitcap_engine_destroy(h)


def test_workspace_holds_the_staged_rows(L):
    """The copy of the forced ids and the per-token buffer are rows of the layout table: the size callers ask for covers them
    (max_length * 12 bytes per sequence, each padded to 256), and layouts without a greedy loop do not carry them."""
    lib = L.lib
    w = lambda B, **kw: lib.vitcap_engine_workspace_bytes(B, C.byref(L.gen_opts(**kw)))
    assert w(64, max_length=40) - w(64) >= 64 * 20 * 12
    assert w(2, seqs_per_image=3) > w(2) and w(1) % 256 == 0


def test_forced_sampler_reproduces_the_oracles_greedy_run(L, sd_t):
    """The oracle's own greedy ids, fed back through greedy_incremental(sampler=forced_sampler(ids)), give the same ids and
    log-probs: forcing what the free run chose changes nothing.  Two images."""
    from oracle import vitcap_oracle as O
    from vitcap_amd import weights as W
    img = torch.from_numpy(W.gen_image_batch(2, 1234))
    with torch.no_grad():
        ids, lp = O.greedy_incremental(sd_t, img)
        forced = ids[:, 0].clone()
        forced[:, 0] = -1
        # an unfinished row's last column holds the [SEP] the max-length rule wrote, not the token chosen there: left free
        forced[:, -1] = -1
        ids_f, lp_f = O.greedy_incremental(sd_t, img, sampler=forced_sampler(forced))
    assert torch.equal(ids_f, ids)
    np.testing.assert_allclose(lp_f.numpy(), lp.numpy(), rtol=0, atol=1e-6)
