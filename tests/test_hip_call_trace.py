"""Which engine entry points every public call of ImageCaptioning reaches, in which order and under which options: that decides speed
and hipGraph use, and no result-level test sees it.  The name `lib` in vitcap_amd.model is replaced by a proxy that forwards everything
and writes down the enqueueing calls, their names without the `vitcap_engine_` prefix:

* generate* / encode* / prefill* / decode* / tags: (name, num_beams, seqs_per_image, use_graph) of the options struct behind the byref
  argument;
* score_req: (name, kind, encode, caps_per_image) of the request.

EXPECTED is a literal, recorded with this same recorder (trace_of below) on the tree before run() / _run_masked() and the hand-written
marshalling of the analysis calls were folded into one call path.  Nothing here looks at results: tests/test_hip_*.py do, and this file
counts for nothing in the coverage ledger of tests/test_cabi.py."""
import re

import pytest
import torch

from vitcap_amd import _lib as L
from vitcap_amd import weights as W
from vitcap_amd.regions import grid_regions

pytestmark = pytest.mark.gpu

TRACED = re.compile(r'vitcap_engine_((generate|encode|prefill|decode)\w*|tags|score_req)$')


class Recorder(object):
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not TRACED.match(name):
            return fn

        def traced(*args):
            short = name[len('vitcap_engine_'):]
            if short == 'score_req':
                r = args[1]._obj
                self.calls.append((short, r.kind, r.encode, r.caps_per_image))
            else:
                o = [a._obj for a in args if isinstance(getattr(a, '_obj', None), L.GenOpts)][0]
                self.calls.append((short, o.num_beams, o.seqs_per_image, o.use_graph))
            return fn(*args)
        return traced


def trace_of(monkeypatch, call, s):
    import vitcap_amd.model as M
    s.m.generate(s.img)      # not traced: slot 0 holds a plain encoding, whichever call ran before (a patch-removed one is refused by some)
    rec = Recorder(M.lib)
    monkeypatch.setattr(M, 'lib', rec)
    call(s)
    torch.cuda.synchronize()
    return rec.calls


class Setup(object):
    def __init__(self):
        from vitcap_amd.model import ImageCaptioning
        self.m = ImageCaptioning(tie_weights=True).load_recipe(0).eval()
        self.m.pack('cuda:0')
        self.img = torch.from_numpy(W.gen_image_batch(2, 4321)).cuda().contiguous()
        ids, _ = self.m.generate(self.img)
        self.cap = ids.view(2, -1).cpu()
        self.prefix = self.cap[:, 1:3].clone()
        self.vis = torch.ones(2, 578, dtype=torch.bool)
        self.vis4 = torch.ones(4, 578, dtype=torch.bool)
        self.present = torch.ones(2, 24, 24, dtype=torch.bool)
        self.g2, self.g3 = grid_regions(2), grid_regions(3)


@pytest.fixture(scope='module')
def s():
    assert torch.cuda.is_available()
    return Setup()


CALLS = {
    'generate': lambda s: s.m.generate(s.img),
    'generate(want_tags)': lambda s: s.m.generate(s.img, want_tags=True),
    'generate(prefix_ids)': lambda s: s.m.generate(s.img, prefix_ids=s.prefix),
    'generate(want_token_logprobs)': lambda s: s.m.generate(s.img, want_token_logprobs=True),
    'generate(visible)': lambda s: s.m.generate(s.img, visible=s.vis),
    'generate_multi(2)': lambda s: s.m.generate_multi(s.img, 2),
    'generate_multi(2, want_last)': lambda s: s.m.generate_multi(s.img, 2, want_last=True),
    'generate_multi(2, visible)': lambda s: s.m.generate_multi(s.img, 2, visible=s.vis4),
    'generate_beam(3)': lambda s: s.m.generate_beam(s.img, 3),
    'generate_beam(3, visible)': lambda s: s.m.generate_beam(s.img, 3, visible=s.vis),
    'score': lambda s: s.m.score(s.img, s.cap),
    'score(one_pass)': lambda s: s.m.score(s.img, s.cap, one_pass=True),
    'score_encoded': lambda s: (s.m.generate(s.img), s.m.score_encoded(s.cap)),
    'score_masked': lambda s: s.m.score_masked(s.img, s.cap, s.vis),
    'score_masked(one_pass=False)': lambda s: s.m.score_masked(s.img, s.cap, s.vis, one_pass=False),
    'attention_maps': lambda s: s.m.attention_maps(s.img, s.cap),
    'attention_maps_encoded': lambda s: (s.m.generate(s.img), s.m.attention_maps_encoded(s.cap)),
    'caption_with_maps': lambda s: s.m.caption_with_maps(s.img),
    'alternatives': lambda s: s.m.alternatives(s.img, s.cap),
    'caption_with_alternatives': lambda s: s.m.caption_with_alternatives(s.img),
    'occlusion_maps(window=12)': lambda s: s.m.occlusion_maps(s.img, s.cap, window=12),
    'caption_with_occlusion(window=12)': lambda s: s.m.caption_with_occlusion(s.img, window=12),
    'visual_gain': lambda s: s.m.visual_gain(s.img, s.cap),
    'caption_regions(grid 2)': lambda s: s.m.caption_regions(s.img, s.g2),
    'caption_regions(grid 3)': lambda s: s.m.caption_regions(s.img, s.g3),
    'caption_regions_encoded': lambda s: (s.m.generate(s.img), s.m.caption_regions_encoded(s.g2)),
    'caption_with_regions': lambda s: s.m.caption_with_regions(s.img, s.g2),
    'caption_regions_beam(3)': lambda s: s.m.caption_regions_beam(s.img, s.g2, 3),
    'caption_with_regions_beam(3)': lambda s: s.m.caption_with_regions_beam(s.img, s.g2, 3),
    'tag_patches': lambda s: s.m.tag_patches(s.img, s.present),
    'caption_patches(want_tags)': lambda s: s.m.caption_patches(s.img, s.present, want_tags=True),
    'score_patches': lambda s: s.m.score_patches(s.img, s.cap, s.present),
    'caption_crops(grid 2)': lambda s: s.m.caption_crops(s.img, s.g2),
    'encoder_attention(blocks=[0])': lambda s: s.m.encoder_attention(s.img, blocks=[0]),
    'tag_rollout': lambda s: s.m.tag_rollout(s.img),
    'rollout_maps': lambda s: s.m.rollout_maps(s.img, s.cap),
    'caption_with_rollout': lambda s: s.m.caption_with_rollout(s.img),
}

EXPECTED = {
    'generate': [
        ('generate', 1, 1, 0),
    ],
    'generate(want_tags)': [
        ('generate', 1, 1, 0),
    ],
    'generate(prefix_ids)': [
        ('generate_forced', 1, 1, 0),
    ],
    'generate(want_token_logprobs)': [
        ('generate_forced', 1, 1, 0),
    ],
    'generate(visible)': [
        ('generate_masked', 1, 1, 0),
    ],
    'generate_multi(2)': [
        ('generate', 1, 2, 0),
    ],
    'generate_multi(2, want_last)': [
        ('encode', 1, 2, 0),
        ('prefill', 1, 2, 0),
        ('decode', 1, 2, 0),
    ],
    'generate_multi(2, visible)': [
        ('generate_masked', 1, 2, 0),
    ],
    'generate_beam(3)': [
        ('generate', 3, 1, 0),
    ],
    'generate_beam(3, visible)': [
        ('generate_beam_masked', 3, 1, 0),
    ],
    'score': [
        ('generate_forced', 1, 1, 0),
    ],
    'score(one_pass)': [
        ('score_req', 0, 1, 1),
    ],
    'score_encoded': [
        ('generate', 1, 1, 0),
        ('score_req', 0, 0, 1),
    ],
    'score_masked': [
        ('score_req', 1, 1, 1),
    ],
    'score_masked(one_pass=False)': [
        ('generate_masked', 1, 1, 0),
    ],
    'attention_maps': [
        ('score_req', 2, 1, 1),
    ],
    'attention_maps_encoded': [
        ('generate', 1, 1, 0),
        ('score_req', 2, 0, 1),
    ],
    'caption_with_maps': [
        ('encode', 1, 1, 0),
        ('prefill', 1, 1, 0),
        ('decode', 1, 1, 0),
        ('score_req', 2, 0, 1),
    ],
    'alternatives': [
        ('score_req', 3, 1, 1),
    ],
    'caption_with_alternatives': [
        ('encode', 1, 1, 0),
        ('prefill', 1, 1, 0),
        ('decode', 1, 1, 0),
        ('score_req', 3, 0, 1),
    ],
    'occlusion_maps(window=12)': [
        ('score_req', 1, 1, 5),
    ],
    'caption_with_occlusion(window=12)': [
        ('encode', 1, 1, 0),
        ('prefill', 1, 1, 0),
        ('decode', 1, 1, 0),
        ('score_req', 1, 0, 5),
    ],
    'visual_gain': [
        ('score_req', 1, 1, 2),
    ],
    'caption_regions(grid 2)': [
        ('generate_masked', 1, 4, 0),
    ],
    'caption_regions(grid 3)': [
        ('generate_masked', 1, 8, 0),
        ('decode_masked', 1, 1, 0),
    ],
    'caption_regions_encoded': [
        ('generate', 1, 1, 0),
        ('decode_masked', 1, 4, 0),
    ],
    'caption_with_regions': [
        ('encode', 1, 1, 0),
        ('prefill', 1, 1, 0),
        ('decode', 1, 1, 0),
        ('decode_masked', 1, 4, 0),
    ],
    'caption_regions_beam(3)': [
        ('encode', 3, 1, 0),
        ('prefill', 3, 1, 0),
        ('decode_beam_masked', 3, 1, 0),
        ('decode_beam_masked', 3, 1, 0),
        ('decode_beam_masked', 3, 1, 0),
        ('decode_beam_masked', 3, 1, 0),
    ],
    'caption_with_regions_beam(3)': [
        ('encode', 3, 1, 0),
        ('prefill', 3, 1, 0),
        ('decode', 3, 1, 0),
        ('decode_beam_masked', 3, 1, 0),
        ('decode_beam_masked', 3, 1, 0),
        ('decode_beam_masked', 3, 1, 0),
        ('decode_beam_masked', 3, 1, 0),
    ],
    'tag_patches': [
        ('encode_patches', 1, 1, 0),
        ('prefill_patches', 1, 1, 0),
        ('tags', 1, 1, 0),
    ],
    'caption_patches(want_tags)': [
        ('encode_patches', 1, 1, 0),
        ('prefill_patches', 1, 1, 0),
        ('tags', 1, 1, 0),
        ('decode_masked', 1, 1, 0),
    ],
    'score_patches': [
        ('encode_patches', 1, 1, 0),
        ('prefill_patches', 1, 1, 0),
        ('score_req', 1, 0, 1),
    ],
    'caption_crops(grid 2)': [
        ('encode_patches', 1, 1, 0),
        ('prefill_patches', 1, 1, 0),
        ('tags', 1, 1, 0),
        ('decode_masked', 1, 1, 0),
    ],
    'encoder_attention(blocks=[0])': [
        ('encode_maps', 1, 1, 0),
        ('prefill', 1, 1, 0),
    ],
    'tag_rollout': [
        ('encode_maps', 1, 1, 0),
        ('prefill', 1, 1, 0),
        ('tags', 1, 1, 0),
    ],
    'rollout_maps': [
        ('encode_maps', 1, 1, 0),
        ('prefill', 1, 1, 0),
        ('score_req', 2, 0, 1),
    ],
    'caption_with_rollout': [
        ('encode_maps', 1, 1, 0),
        ('prefill', 1, 1, 0),
        ('decode', 1, 1, 0),
        ('score_req', 2, 0, 1),
    ],
}


@pytest.mark.parametrize('name', list(CALLS))
def test_trace(s, monkeypatch, name):
    with torch.no_grad():
        got = trace_of(monkeypatch, CALLS[name], s)
    assert got == EXPECTED[name], name


def test_every_call_has_a_recorded_trace():
    assert sorted(CALLS) == sorted(EXPECTED) and all(EXPECTED.values())
