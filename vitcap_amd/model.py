"""Host-side mirror of the reference's model surface for the captioning hot path.

``ImageCaptioning`` here plays the role of the reference's
``src/pipelines/tagger_caption_uni_pipeline_expanding_bertemb.py:23-189 ImageCaptioning`` wrapping
``src/layers/bert/modeling_bert.py:695 ViTCAP`` and the ``InputAsDict``-wrapped timm ViT patch embedder:

* same ``state_dict()`` key names and shapes, so a reference checkpoint loads as is;
* same call contract: ``forward(data: dict)`` -> at test time ``(ids int64 (B,1,20), logprobs fp32 (B,1))``.

All arithmetic runs in the hand-written HIP kernels of libvitcap_hip.so through one C-ABI engine call
per batch; PyTorch only owns the memory.  There is no CPU/eager fallback.
"""
import ctypes as C

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import weights as W
from ._lib import lib, check, VitcapError


class _Node(nn.Module):
    """Anonymous container: the parameter tree only has to reproduce the reference's key names."""


def _build_tree(root, spec, tie_weights):
    params = {}
    for key, (shape, _kind) in spec.items():
        parts = key.split('.')
        mod = root
        for p in parts[:-1]:
            if p not in mod._modules:
                mod.add_module(p, _Node())
            mod = mod._modules[p]
        if tie_weights and key == W.TIED_DST:
            prm = params[W.TIED_SRC]           # same Parameter object, as _tie_or_clone_weights does
        else:
            prm = nn.Parameter(torch.zeros(shape, dtype=torch.float32), requires_grad=False)
        mod.register_parameter(parts[-1], prm)
        params[key] = prm
    return params


_ROLE_STREAMS = {}


def role_stream(dev, role, make):
    """One stream per (device, role) for the life of the PROCESS.  torch hands out its pool streams round-robin and HIP maps streams onto
    a few hardware queues (GPU_MAX_HW_QUEUES, default 4): with a fresh pair of streams per model object, every new model of a process drew
    another arrangement, and the ones that put the encoder chain and the decode chain (or the loader's copies) on one queue ran the 2-slot
    pipeline at half its rate (profiles/r05_hw_queue_aliasing.txt).  Streams are only ever added, never handed back."""
    dev = torch.device(dev)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), role)
    s = _ROLE_STREAMS.get(key)
    if s is None:
        s = _ROLE_STREAMS[key] = make()
    return s


def _encode_stream(dev):
    """The pipeline's encoder stream.  VITCAP_ENC_CUS = n < 256 (experiment, docs/LAB_r01_r04.md 4.2 vi) confines it to the CUs of the
    low n mask bits (hipExtStreamCreateWithCUMask: bit i -> XCD i % 8), which leaves 256 - n CUs that the encoder's GEMM
    workgroups never occupy for the decode chain's dependent launches to start on."""
    import os
    n = int(os.environ.get('VITCAP_ENC_CUS', '256'))
    if n >= 256:
        return torch.cuda.Stream(dev)
    words = (C.c_uint32 * 8)()
    for cu in range(n):
        words[cu // 32] |= 1 << (cu % 32)
    hip = C.CDLL('libamdhip64.so')
    h = C.c_void_p()
    with torch.cuda.device(dev):
        rc = hip.hipExtStreamCreateWithCUMask(C.byref(h), 8, words)
    if rc != 0:
        raise RuntimeError('hipExtStreamCreateWithCUMask failed: %d' % rc)
    return torch.cuda.ExternalStream(h.value, device=dev)


class _Pending(object):
    """Handle of one batch in flight in ImageCaptioning.generate_async."""

    def __init__(self, ids, lp, event, keep):
        self.ids, self.lp, self.event, self._keep = ids, lp, event, keep

    def wait(self, stream=None):
        """Makes `stream` (default: the current stream) wait for this batch, without blocking the host."""
        (stream or torch.cuda.current_stream(self.ids.device)).wait_event(self.event)
        return self.ids, self.lp

    def result(self):
        self.event.synchronize()
        self._keep = None
        return self.ids, self.lp


class _PatchEncoded(tuple):
    """self._encoded[slot] after a patch-removed encoding (ImageCaptioning.tag_patches / caption_patches / ...): the usual (opts, B)
    plus `words`, the packed presence rows (B, 19) on the device.  Any later encoding on the slot stores a plain tuple again."""
    words = None


def _p(t):
    """Tensor -> the pointer argument of an engine call; None stays None (an output the call does not want)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(s=None):
    """The HIP stream argument of an engine call: `s`, or the current stream."""
    return C.c_void_p((torch.cuda.current_stream() if s is None else s).cuda_stream)


# How each generate() option that some call is not built for shows in the merged options (test_extra_input + overrides).
_OPTION_SET = {'num_beams': lambda v: int(v or 1) > 1, 'use_cbs': bool, 'tag_visible': lambda v: int(v or 0) > 0, 'do_sample': bool,
               'use_graph': bool, 'repetition_penalty': lambda v: float(v or 1) != 1.0}

# Family of calls -> (why, the options it refuses, in the order they are looked at).  The rows differ for historical reasons (the
# caption_with_* calls let tag_visible through to their greedy pass, only the one-pass scorer looks at repetition_penalty, ...):
# tests/test_refusal_matrix_cpu.py pins them as they are.
_REFUSED = {
    'forced': ('forced tokens under beam search are not built: the greedy / sampling loop takes them, not', ('num_beams', 'use_cbs')),
    'visible': ('a visibility mask is not built for', ('num_beams', 'use_cbs', 'tag_visible')),
    'visible_beam': ('a visibility mask under beam search is not built for', ('use_cbs', 'tag_visible', 'do_sample', 'use_graph')),
    'one_pass': ('a caption is scored in one pass, not searched or drawn: not built for',
                 ('num_beams', 'use_cbs', 'repetition_penalty', 'tag_visible', 'do_sample')),
    'greedy': ('it runs greedy captions only: not built for', ('num_beams', 'use_cbs', 'do_sample')),
    'regions': ('region captions are greedy, under a visibility mask: not built for', ('do_sample', 'num_beams', 'use_cbs', 'tag_visible')),
    'patches': ('patch removal (greedy loop and one-pass scorer, this call\'s own mask) is not built for',
                ('use_cbs', 'num_beams', 'tag_visible', 'use_graph', 'do_sample')),
    'rollout': ('the encoder rollout (a plain greedy / one-pass pass, the call\'s own launches) is not built for',
                ('use_cbs', 'num_beams', 'tag_visible', 'do_sample', 'use_graph')),
}


def _refuse_options(who, family, te):
    """Raises NotImplementedError naming `who`, the option and its value for the first option of `te` the family is not built for."""
    why, names = _REFUSED[family]
    for name in names:
        if _OPTION_SET[name](te.get(name)):
            raise NotImplementedError('%s: %s %s (got %s=%r)' % (who, why, name, name, te[name]))


class ImageCaptioning(nn.Module):
    """ViT-B/16-384 + tag head + 4-layer BERT caption decoder, greedy decode on MI355X."""

    def __init__(self, tie_weights=True, tagemb='cls', test_extra_input=None, cfg=None):
        super().__init__()
        self.tie_weights = tie_weights
        self.tagemb = tagemb
        self.cfg = cfg
        # decode kwargs the reference passes at test time (..._bertemb.py:588-608)
        self.test_extra_input = dict(is_decode=True, do_sample=False, bos_token_id=101, pad_token_id=0,
                                     eos_token_ids=[102], mask_token_id=103, add_od_labels=True,
                                     od_labels_start_posid=20, max_length=20, num_beams=1, temperature=1,
                                     top_k=0, top_p=1, repetition_penalty=1, length_penalty=1,
                                     num_return_sequences=1, num_keep_best=1)
        if test_extra_input:
            self.test_extra_input.update(test_extra_input)
        self._params = _build_tree(self, W.state_dict_spec(), tie_weights)
        self._engine = None
        self._packed = None
        self._ws = {}
        self._score_ws = {}      # slot -> the one-pass scorer's workspace (vitcap_engine_score)
        self._encoded = {}       # slot -> (opts, B) of the call whose encoder pass + prefill the slot's workspace holds
        self.last_tags = None

    # ---------------------------------------------------------------- weights
    def load_recipe(self, seed=0, vbias_std=None, bf16_exact=True):
        sd = W.make_state_dict(seed=seed, tie_weights=self.tie_weights, vbias_std=vbias_std, bf16_exact=bf16_exact)
        with torch.no_grad():
            for k, v in sd.items():
                self._params[k].copy_(torch.from_numpy(v))
        self._packed = None
        return self

    def load_state_dict(self, state_dict, strict=True):
        res = super().load_state_dict(state_dict, strict=strict)
        self._packed = None
        return res

    def _t(self, key):
        return self._params[key].detach()

    def bind_weights(self, source, keep, dev):
        """Fills a vitcap_weights by walking W.weights_table() -- `source(field)` gives the device tensor behind a field, or None for
        an optional field that stays null -- and binds it to the engine (created on first use).  `keep` holds what must outlive it."""
        w, done = L.Weights(), {}
        for f in W.weights_table():
            t = done[f.tied_to] if (f.tied_to and self._params[W.TIED_DST] is self._params[W.TIED_SRC]) else source(f)
            if t is None:
                assert f.optional, f.path
                continue
            done[f.path] = t
            dst = w
            for step in f.path[:-1]:
                dst = dst[step] if isinstance(step, int) else getattr(dst, step)
            setattr(dst, f.path[-1], _p(t))
        if self._engine is None:
            h = C.c_void_p()
            check(lib.vitcap_engine_create(C.byref(h)), 'engine_create')
            self._engine = h
        check(lib.vitcap_engine_bind_weights(self._engine, C.byref(w)), 'bind_weights')
        self._packed = (w, keep, dev)
        return self

    def pack(self, device='cuda'):
        """Re-lay the checkpoint tensors for the kernels (bf16 matrices, fused decoder QKV, padded vocab)."""
        dev = torch.device(device)
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        keep = []

        def convert(f):
            if f.optional and self.tagemb == 'cls':
                # bert.extra_embeddings: the tag rows' embedding under branch B of modeling_bert.py:1484-1485 (only read when the tag
                # tokens are visible to the caption, vitcap_gen_opts.tag_visible > 0)
                return None
            t = torch.cat([self._t(k) for k in f.keys], 0) if len(f.keys) > 1 else self._t(f.keys[0])
            if f.shape is not None:
                t = t.reshape(f.shape)
            if f.pad is not None:
                o = torch.zeros((f.pad,) + tuple(t.shape[1:]), dtype=torch.float32)
                o[:t.shape[0]] = t
                t = o
            t = t.to(device=dev, dtype=torch.float32)
            t = (t.to(torch.bfloat16) if f.kind == 'mat' else t).contiguous()
            keep.append(t)
            return t

        return self.bind_weights(convert, keep, dev)

    def __del__(self):
        try:
            if self._engine is not None:
                lib.vitcap_engine_destroy(self._engine)
        except Exception:
            pass

    # ---------------------------------------------------------------- forward
    def _workspace(self, B, dev, slot=0, opts=None, wait=None, keep=False):
        """One workspace per slot: concurrent generate() calls on different HIP streams use different slots.  `wait`: event of
        the slot's in-flight work, waited for before a larger buffer replaces the old one (the caching allocator may hand the
        old block to another stream at once).  keep: a larger buffer starts as a copy of the old one (a decode on the slot's prefill
        with more sequences per image than the call that encoded)."""
        need = lib.vitcap_engine_workspace_bytes(B, C.byref(opts) if opts is not None else None)
        if need == 0:
            check(lib.vitcap_gen_opts_check(C.byref(opts)), 'gen_opts')
        ws = self._ws.get(slot)
        if ws is None or ws.numel() < need or ws.device != dev:
            if ws is not None and wait is not None:
                wait.synchronize()
            old, ws = ws, torch.empty(need, dtype=torch.uint8, device=dev)
            if keep and old is not None and old.device == dev:
                ws[:old.numel()].copy_(old)      # the per-image buffers come first in the layout: the prefill stays where it was
            self._ws[slot] = ws
        return ws, need

    # ---- options: test_extra_input (the kwargs ViTCAP.generate receives, ..._bertemb.py:588-608) -> vitcap_gen_opts
    def gen_options(self, gemm_mode=L.GEMM_AUTO, use_graph=None, **over):
        """Validated vitcap_gen_opts for the current test_extra_input (+ overrides).  Raises for generate() options this build
        does not implement instead of silently ignoring them; used by forward() AND by the pipeline's predict loop."""
        te = dict(self.test_extra_input)
        te.update(over)
        cbs = None
        if te.get('use_cbs', False):
            # ViTCAP.generate(use_cbs=True, fsm=, num_constraints=, min_constraints_to_satisfy=) (modeling_bert.py:932-933, 949-953,
            # 1035-1057).  The reference's pipeline sets use_cbs / min_constraints_to_satisfy (..._bertemb.py:175-179) but nothing in
            # it ever supplies `fsm`: there generate() dies on `fsm.shape`; here the missing tensors are named.
            fsm, ncons = te.get('fsm'), te.get('num_constraints')
            if fsm is None or ncons is None:
                raise ValueError('use_cbs needs `fsm` (B, S, S, %d) uint8 and `num_constraints` (B,) next to it (vitcap_amd.cbs.batch_fsm); '
                                 'the reference reads fsm.shape at modeling_bert.py:952' % L.VOCAB)
            if fsm.dim() != 4 or fsm.shape[1] != fsm.shape[2] or fsm.shape[3] != L.VOCAB:
                raise AssertionError('fsm must be (B, S, S, %d), got %s (modeling_bert.py:953)' % (L.VOCAB, tuple(fsm.shape)))
            if not (fsm.is_cuda and ncons.is_cuda and fsm.is_contiguous() and fsm.dtype in (torch.uint8, torch.bool)):
                raise ValueError('fsm / num_constraints must be contiguous device tensors (uint8 / int64)')
            ncons = ncons.to(torch.int64).contiguous()
            cbs = (fsm, ncons)
            self._cbs_keep = cbs                       # the option struct holds raw pointers into these
        if not te.get('add_od_labels', True):
            # without the 50 od slots ViTSplitCLSEmbModel.forward has no rows to write its tag embeddings over
            # (`embedding_output[:, -pred_topk.shape[1]:] = tag_embedding`, modeling_bert.py:1467 / 1489) and the reference fails
            raise NotImplementedError('add_od_labels=False: the reference model needs the 50 tag slots behind the caption')
        eos = te.get('eos_token_ids', [102])
        eos = [int(x) for x in eos] if isinstance(eos, (list, tuple)) else [int(eos)]
        if not 1 <= len(eos) <= 4:
            raise NotImplementedError('eos_token_ids must hold 1..4 ids in this build (got %r)' % (eos,))
        nb, keep = int(te.get('num_beams', 1) or 1), int(te.get('num_keep_best', 1) or 1)
        nret = int(te.get('num_return_sequences', 1) or 1)
        do_sample = bool(te.get('do_sample', False))
        if keep != 1 and nb == 1:
            # modeling_utils.py:790: "cannot generate >1 sentences in greedy search"
            raise AssertionError('cannot generate >1 sentences in greedy search (num_keep_best > 1 needs num_beams > 1)')
        if len(eos) > 1 and nb > 1:
            # with several EOS ids more than num_beams of the 2*num_beams candidates can be EOS words and the reference's own
            # `assert len(next_sent_beam) == num_beams` fires (modeling_utils.py:1037): only the greedy / sampling loop takes a list
            raise NotImplementedError('several eos_token_ids need num_beams == 1 (the reference\'s beam search asserts with them)')
        if nret > 1 and (not do_sample or nb > 1):
            raise NotImplementedError('num_return_sequences > 1 needs do_sample and num_beams == 1 (the reference asserts the same)')
        ml = int(te.get('max_length', L.MAXLEN))
        if not 2 <= ml <= L.MAXLEN_CAP:
            raise NotImplementedError('max_length must be 2..%d in this build (got %d)' % (L.MAXLEN_CAP, ml))
        sp = L.SampleParams(int(do_sample), float(te.get('temperature', 1) or 1), int(te.get('top_k', 0) or 0),
                            float(te.get('top_p', 1) or 1), int(te.get('seed', 0)) & 0xffffffff)
        if use_graph is None:
            use_graph = bool(te.get('use_graph', False))
        o = L.gen_opts(num_beams=nb, seqs_per_image=min(nret, 8) if nret > 1 else 1, num_keep_best=keep, max_length=ml,
                       bos_token_id=int(te.get('bos_token_id', 101)), eos_token_id=int(eos[0]),
                       pad_token_id=int(te.get('pad_token_id', 0)), mask_token_id=int(te.get('mask_token_id', 103)),
                       length_penalty=float(te.get('length_penalty', 1) or 1),
                       repetition_penalty=float(te.get('repetition_penalty', 1) or 1), sampling=sp, gemm_mode=int(gemm_mode),
                       early_exit=int(bool(te.get('early_exit', True))), use_graph=int(bool(use_graph)),
                       tag_visible=int(te.get('tag_visible', 0) or 0), tagemb_cls=int(self.tagemb == 'cls'),
                       decode_streams=int(te.get('decode_streams', 0) or 0), encode_parts=int(te.get('encode_parts', 0) or 0),
                       eos_extra=eos[1:], tag_pos0=max(int(te.get('od_labels_start_posid', 20) or 0), ml, 20))
        if cbs is not None:
            o.use_cbs, o.cbs_states = 1, int(cbs[0].shape[1])
            o.min_constraints_to_satisfy = int(te.get('min_constraints_to_satisfy', 2))
            o.fsm, o.num_constraints = cbs[0].data_ptr(), cbs[1].data_ptr()
            # the search's optional rules (generate kwargs, modeling_bert.py:933, 1039-1042)
            if te.get('use_hypo', False):
                # upstream cannot run it either: utils_cbs.py:273 indexes a tensor with `beam_id / per_node_beam_size`, a float
                raise NotImplementedError('use_hypo: the reference\'s own hypothesis branch fails on a float tensor index (utils_cbs.py:273)')
            o.cbs_no_repeat = int(bool(te.get('decoding_constraint_flag', False)))
            bad = [int(x) for x in (te.get('bad_ending_ids') or [])]
            if len(bad) > 16:
                raise NotImplementedError('bad_ending_ids: at most 16 ids in this build (got %d)' % len(bad))
            o.cbs_bad_ending = (C.c_int32 * 16)(*(bad + [-1] * (16 - len(bad))))
        check(lib.vitcap_gen_opts_check(C.byref(o)), 'gen_opts')
        return o

    @staticmethod
    def _text_mask_pattern(T, max_length, n_tag, dtype, device):
        """The attention_mask the kernels implement for n_tag visible tag slots (dataset.py:377-390): tril on the caption slots,
        ones on [0:L, L:L+n] and [L:L+n, L:L+n], zeros elsewhere."""
        want = torch.zeros((T, T), dtype=dtype, device=device)
        want[:max_length, :max_length] = torch.tril(torch.ones(max_length, max_length, dtype=dtype, device=device))
        if n_tag:
            want[max_length:max_length + n_tag, max_length:max_length + n_tag] = 1
            want[:max_length, max_length:max_length + n_tag] = 1
        return want

    def check_text_inputs(self, data, max_length=L.MAXLEN, expect_n_tag=None):
        """The text side of the test-time batch (CaptionTensorizer.tensorize_ab at test time, dataset.py:218-219, 326, 377-390;
        consumed by ImageCaptioning.construct_attn_mask ..._bertemb.py:57-85 and ViTCAP.generate modeling_bert.py:955-1001).
        The engine hard-wires the mask STRUCTURE those tensors describe -- caption row i attends caption rows <= i and the 578
        visual tokens, nothing attends the tag slots -- so what the caller hands over is verified against that structure and
        anything else is refused: a different mask can no longer yield a silently wrong caption.

        * attention_mask (B, T, T), T = max_length + od_len: lower-triangular ones on [0:max_length, 0:max_length], zeros
          elsewhere (the 210 ones of SURVEY 8d for max_length 20) -- or, additionally, the first n tag slots visible to every
          caption row and to each other (what tensorize_ab builds for a text_b of n tokens): returns n;
        * token_type_ids: zeros;  masked_pos: not read by generate() beyond slicing;
        * input_ids (B, T): only the od-label slots [max_length:] are read by generate() (modeling_bert.py:959); their
          embeddings are overwritten by the predicted tag tokens (1435-1489) and never attended, so any value is harmless.

        expect_n_tag=None: returns n, read off the mask (host tensors: no GPU involved; device tensors: one host synchronisation).
        expect_n_tag=n (the pipeline's steady state, pipeline.predict): tensors that live on the device are compared with the
        pattern for n ON THEIR STREAM and nothing is read back -- returns (n, flag) with flag a 0-d device bool (True = inputs
        acceptable) that the caller tests when it next synchronises anyway, or None when everything was checked on the host."""
        am = data.get('attention_mask')
        defer = expect_n_tag is not None
        n_tag = int(expect_n_tag) if defer else 0
        flag = None

        def _verdict(ok_tensor, make_error):
            nonlocal flag
            if defer and ok_tensor.is_cuda:
                flag = ok_tensor if flag is None else (flag & ok_tensor)
            elif not bool(ok_tensor):
                raise make_error()

        if am is not None:
            if am.dim() != 3 or am.shape[1] != am.shape[2] or am.shape[1] < max_length:
                raise ValueError('attention_mask must be (B, T, T) with T >= max_length=%d, got %s' % (max_length, tuple(am.shape)))
            T = am.shape[1]
            # tags visible to the caption (a text_b of n tokens, dataset.py:240-252, 387-390): ones on [L0:L0+n, L0:L0+n] and on
            # [0:L0, L0:L0+n]; n is read off the first caption row of the first sample and must describe the whole batch
            if not defer or not am.is_cuda:
                n_tag = int((am[0, 0, max_length:] != 0).sum())
                if defer and n_tag != int(expect_n_tag):
                    raise ValueError('attention_mask shows %d visible tag slots, the batches before it showed %d' % (n_tag, int(expect_n_tag)))
            want = self._text_mask_pattern(T, max_length, n_tag, am.dtype, am.device)
            _verdict((am == want.unsqueeze(0)).all(), lambda: NotImplementedError(
                'attention_mask is neither the test-time seq2seq pattern (tril on the first %d caption slots, zeros elsewhere: '
                'dataset.py:377-390) nor that pattern with the first n tag slots visible to the caption and to each other '
                '(dataset.py:387-390); the HIP engine implements these two mask structures only' % max_length))
            if n_tag > 50 or (n_tag and max_length != L.MAXLEN):
                raise NotImplementedError('tag tokens visible to the caption need max_length == 20 and at most 50 tag slots')
        tt = data.get('token_type_ids')
        if tt is not None:
            _verdict((tt == 0).all(), lambda: NotImplementedError(
                'token_type_ids must be all zero at test time (dataset.py:326); segment-1 text tokens are not built'))
        ii = data.get('input_ids')
        if ii is not None and (ii.dim() != 2 or ii.shape[1] < max_length):
            raise ValueError('input_ids must be (B, T) with T >= max_length=%d, got %s' % (max_length, tuple(ii.shape)))
        for k in ('input_ids', 'attention_mask', 'token_type_ids', 'masked_pos'):
            v = data.get(k)
            if v is not None and v.shape[0] != data['image'].shape[0]:
                raise ValueError('%s has batch %d but image has %d' % (k, v.shape[0], data['image'].shape[0]))
        return (n_tag, flag) if defer else n_tag

    def _check_image(self, image):
        if self._packed is None:
            self.pack(image.device)
        assert image.is_cuda and image.is_contiguous() and tuple(image.shape[1:]) == (3, 384, 384)
        assert image.dtype in (torch.float32, torch.bfloat16)
        return self._packed[2]

    def _out_buffers(self, B, o, dev):
        if o.use_cbs:
            shape = (B, 1)
        elif o.num_beams > 1:
            shape = (B, o.num_keep_best)
        else:
            shape = (B * o.seqs_per_image, 1)
        return (torch.empty(shape + (o.max_length,), dtype=torch.int64, device=dev),
                torch.empty(shape, dtype=torch.float32, device=dev))

    @staticmethod
    def refuse_forced_search(num_beams, use_cbs):
        """Forced tokens (a caption prefix, a caption to score) exist for the greedy / sampling loop only."""
        _refuse_options('prefix_ids / forced tokens', 'forced', dict(num_beams=num_beams, use_cbs=use_cbs))

    def _refuse(self, who, family, over=None):
        """What a family of calls (_REFUSED) is not built for, looked up in test_extra_input + `over` and refused by the option's
        name, before the GPU is touched.  -> the merged options."""
        te = dict(self.test_extra_input)
        te.update(over or {})
        _refuse_options(who, family, te)
        return te

    def refuse_visible(self, who, over=None):
        """A visibility mask (`visible` / regions) exists for the greedy / sampling loop without visible tags."""
        self._refuse(who, 'visible', over)

    def _greedy_options(self, over, no_graph=False, drop=(), **fixed):
        """The validated options of a call that decides the search itself: greedy unless `fixed` says otherwise, without a hipGraph
        when asked; `over` gives the rest, whatever it says about the fixed keys (and those of `drop`) is left out."""
        fixed = dict(dict(num_beams=1, do_sample=False, num_return_sequences=1, num_keep_best=1), **fixed)
        if no_graph:
            fixed['use_graph'] = False
        return self.gen_options(**fixed, **{k: v for k, v in over.items() if k not in fixed and k not in drop})

    def _head(self, image, B, opts, ws, need):
        """The leading arguments every staged (image None) or whole engine call shares."""
        return (self._engine,) + (() if image is None else (_p(image), int(image.dtype == torch.bfloat16))) + (B, C.byref(opts), _p(ws), need)

    def _encode_prefill(self, image, opts, ws, need, stream):
        B = image.shape[0]
        check(lib.vitcap_engine_encode(*self._head(image, B, opts, ws, need), stream), 'engine_encode')
        check(lib.vitcap_engine_prefill(*self._head(None, B, opts, ws, need), stream), 'engine_prefill')

    def _decode(self, kind, image, B, opts, ws, need, ids, lp, tail, forced=None, score_forced=0, tok_lp=None, vis=None, stream=None):
        """One call of the decode family: vitcap_engine_generate[_kind] on `image`, or with image None vitcap_engine_decode[_kind] on
        the prefill the workspace holds; kind '' | 'forced' | 'masked' | 'beam_masked'.  tail: (last,) of a staged call, (tag_logits,
        tag_topk) of a whole one, tensors or None.  Every kind but '' takes the forced ids and gives the per-token log-probs."""
        fn = 'engine_' + ('decode' if image is None else 'generate') + ('_' + kind if kind else '')
        args = self._head(image, B, opts, ws, need) + ((_p(forced), int(score_forced)) if kind else ()) + (_p(ids), _p(lp)) \
            + ((_p(tok_lp),) if kind else ()) + tuple(_p(t) for t in tail) + ((_p(vis),) if kind.endswith('masked') else ()) \
            + (_stream() if stream is None else stream,)
        check(getattr(lib, 'vitcap_' + fn)(*args), fn)

    def run(self, image, opts, want_tags=False, slot=0, want_last=False, forced=None, score_forced=0, want_token_logprobs=False,
            vis=None):
        """One vitcap_engine_generate call on the current stream under `opts` (a vitcap_gen_opts from gen_options()).
        forced (rows, max_length) int64 / score_forced: vitcap_amd.forced.pack_forced; with want_token_logprobs the per-token
        log-probs (rows, max_length) are returned last.  Either one makes it a vitcap_engine_generate_forced call.
        vis int32 (rows, 19), vitcap_amd.occlusion.pack_visible: visual keys hidden per sequence, a vitcap_engine_generate_masked
        call (no hipGraph: the call sets use_graph = 0).  With vis, image None decodes on the prefill the last call left on `slot`.
        want_last (or image None) takes the staged path -- vitcap_engine_encode + _prefill, then vitcap_engine_decode[_forced |
        _masked] -- and returns the token chosen at the last position behind (ids, logprobs)."""
        use_forced = forced is not None or want_token_logprobs
        if use_forced:
            self.refuse_forced_search(opts.num_beams, opts.use_cbs)
        if vis is not None:
            _refuse_options('run', 'visible', dict(num_beams=opts.num_beams, use_cbs=opts.use_cbs, tag_visible=opts.tag_visible))
            opts.use_graph = 0
        if image is not None or vis is None:
            dev, B = self._check_image(image), image.shape[0]
        else:
            if slot not in self._encoded:
                raise RuntimeError('no encoded images on slot %r (call run / generate / score on it first)' % (slot,))
            self._refuse_patch_slot('run(image=None)', slot)
            o_last, B = self._encoded[slot]
            if opts.max_length != o_last.max_length or o_last.tag_visible > 0:
                raise ValueError('the last call on slot %r ran other options (max_length / tags)' % (slot,))
            dev = self._packed[2]
        rows = B * opts.seqs_per_image
        if vis is not None:
            if tuple(vis.shape) != (rows, 19):
                raise ValueError('the packed visibility mask must be (%d, 19), got %s' % (rows, tuple(vis.shape)))
            # read in place by the enqueued kernels: allocated and released on this stream, so the block is not reused before them
            vis = vis.to(device=dev, dtype=torch.int32).contiguous()
        tok_lp = None
        if forced is not None:
            if tuple(forced.shape) != (rows, opts.max_length):
                raise ValueError('forced ids must be (%d, %d), got %s' % (rows, opts.max_length, tuple(forced.shape)))
            forced = forced.to(device=dev, dtype=torch.int64).contiguous()
        if want_token_logprobs:
            tok_lp = torch.empty((rows, opts.max_length), dtype=torch.float32, device=dev)
        ws, need = self._workspace(B, dev, slot, opts, keep=image is None)
        ids, lp = self._out_buffers(B, opts, dev)
        extra = (tok_lp,) if want_token_logprobs else ()
        kind = 'masked' if vis is not None else 'forced' if use_forced else ''
        self._encoded[slot] = (opts, B)
        if image is None or want_last:
            # staged: the encoder and the prefill (unless the slot holds them), then the decode loop on their own
            last = torch.empty((rows,), dtype=torch.int64, device=dev) if want_last else None
            if image is not None:
                self._encode_prefill(image, opts, ws, need, _stream())
            self._decode(kind, None, B, opts, ws, need, ids, lp, (last,), forced, score_forced, tok_lp, vis)
            return ((ids, lp, last) if want_last else (ids, lp)) + extra
        tags = (torch.empty((B, L.VOCAB), dtype=torch.float32, device=dev),
                torch.empty((B, 50), dtype=torch.int64, device=dev)) if want_tags else (None, None)
        self._decode(kind, image, B, opts, ws, need, ids, lp, tags, forced, score_forced, tok_lp, vis)
        if want_tags:
            self.last_tags = tags
        self._last = (slot, opts, B)
        return (ids, lp) + extra

    def _visible_words(self, who, visible, rows, keep_cls, over):
        """`visible` of generate / generate_multi -> (packed words or None, `over` with use_graph off); the refusals come first."""
        if visible is None:
            return None, over
        from .occlusion import as_visible, pack_visible
        self.refuse_visible(who, over)
        return pack_visible(as_visible(visible, rows, keep_cls)), dict(over, use_graph=False)

    @staticmethod
    def _prefix_forced(prefix_ids, B, K, max_length):
        """prefix_ids (B, P) -- one prefix per image, shared by its K sequences -- or (B*K, P) -> pack_forced's (forced, 0)."""
        from .forced import pack_forced
        if prefix_ids is None:
            return None, 0
        p = torch.as_tensor(prefix_ids)
        if K > 1 and p.dim() == 2 and p.shape[0] == B:
            p = p.repeat_interleave(K, 0)
        return pack_forced(prefix_ids=p, rows=B * K, max_length=max_length)

    def generate(self, image, want_tags=False, slot=0, prefix_ids=None, want_token_logprobs=False, visible=None, keep_cls=True, **over):
        """Greedy captions.  image: (B,3,384,384) fp32 or bf16 on the GPU, normalised with mean=.5/std=.5.
        prefix_ids (B, P), -1-padded: the captions start with these tokens (positions 1..P; they do not enter the score, like a
        reference loop started at cur_len = P).  want_token_logprobs: returns (ids, logprobs, token_logprobs (B, L)).
        visible: as score_masked takes it, one row per image -- (B, 578) in cache order or a (B, 24, 24) patch grid (the two cls
        columns then visible iff keep_cls): the caption is written with the other visual tokens hidden from it in all four decoder
        layers, the reference's attention_mask zeros on caption rows / visual columns (modeling_bert.py:1498-1501).  The mask hides
        visual TOKENS from the CAPTION; the encoder has seen the whole image.  Not built with beams, CBS or visible tags
        (NotImplementedError); no hipGraph is used (the call sets use_graph = 0)."""
        vis, over = self._visible_words('generate', visible, image.shape[0], keep_cls, over)
        o = self.gen_options(num_beams=1, do_sample=False, num_return_sequences=1, num_keep_best=1, **over)
        forced, sf = self._prefix_forced(prefix_ids, image.shape[0], 1, o.max_length)
        return self.run(image, o, want_tags=want_tags, slot=slot, forced=forced, score_forced=sf, want_token_logprobs=want_token_logprobs,
                        vis=vis)

    def generate_multi(self, image, seqs_per_image, slot=0, want_last=False, prefix_ids=None, want_token_logprobs=False, visible=None,
                       keep_cls=True, **over):
        """`seqs_per_image` sampled sequences per image (num_return_sequences of ViTCAP.generate): the encoder and the
        visual prefill run once per image, the sequences of an image share its visual K/V.  Returns (ids (B*n,1,L),
        logprobs (B*n,1)) image-major -- the same sequences generate() gives on the n-times repeated batch -- and, with
        want_last, the token chosen at the last position (before the forced [SEP]) of every sequence.
        prefix_ids (B, P) or (B*n, P) / want_token_logprobs: as generate(); the per-token log-probs come last.
        visible: as generate(), one row per SEQUENCE ((B*n, 578) or (B*n, 24, 24)): the sequences of an image may see different parts."""
        n = min(int(seqs_per_image), 8) if int(seqs_per_image) > 1 else 1      # gen_options' sequences per image
        vis, over = self._visible_words('generate_multi', visible, image.shape[0] * n, keep_cls, over)
        o = self.gen_options(num_beams=1, num_keep_best=1, num_return_sequences=int(seqs_per_image), do_sample=True, **over)
        forced, sf = self._prefix_forced(prefix_ids, image.shape[0], o.seqs_per_image, o.max_length)
        return self.run(image, o, slot=slot, want_last=want_last, forced=forced, score_forced=sf, want_token_logprobs=want_token_logprobs,
                        vis=vis)

    def score(self, image, caption_ids, seqs_per_image=1, slot=0, return_ids=False, last_tok=None, one_pass=False, **over):
        """Log-probability of GIVEN captions under the procedure generate() uses: one [MASK] probe per position on the tokens so
        far, log_softmax gathered at the given token, averaged over the positions up to and including the first [SEP]
        (modeling_utils.py:850-877 on given words).  caption_ids (B * seqs_per_image, L) image-major: [CLS] first,
        [SEP]-terminated, 0-padded -- what generate() returns.  The K captions of an image share its encoder pass and visual K/V.
        A [SEP] in the last column of a caption that has not ended before it was written by the max-length rule, not chosen: that
        position is scored on the loop's own choice, or on last_tok[row] when given (vitcap_amd.forced.pack_forced).
        one_pass: every position in ONE pass over a [token rows | probe rows] grid (vitcap_engine_score) instead of max_length - 1
        forced decode steps; up to 32 captions per image; agrees with the stepwise path within the bounds both meet against the
        reference, not bit for bit.  Repetition penalty, visible tags, sampling, beams and CBS are not built for it.
        -> (logprob (rows,), token_logprobs (rows, L)); with return_ids also the ids the loop wrote."""
        from .forced import pack_forced
        K = int(seqs_per_image)
        if one_pass:
            image, B, o, cap, lt, dev = self._score_source('score', image, slot, caption_ids, K, last_tok, over)
            return self._score_one_pass(image, B, o, cap, lt, K, slot, dev, return_ids)
        o = self.gen_options(num_beams=1, do_sample=False, num_return_sequences=1, num_keep_best=1, **over)
        o.seqs_per_image = K
        check(lib.vitcap_gen_opts_check(C.byref(o)), 'gen_opts')
        forced, sf = pack_forced(caption_ids=caption_ids, rows=image.shape[0] * K, max_length=o.max_length, last_tok=last_tok)
        ids, lp, tok_lp = self.run(image, o, slot=slot, forced=forced, score_forced=sf, want_token_logprobs=True)
        return (lp.view(-1), tok_lp, ids) if return_ids else (lp.view(-1), tok_lp)

    def _score_inputs(self, B, caption_ids, K, last_tok, over):
        """Host-side checks of the one-pass scorer, before anything touches the GPU: the engine's refusals by option name
        (NotImplementedError), then pack_forced's checks of the captions.  -> (opts, caption ids (rows, L), last_tok or None)."""
        from .forced import pack_forced
        self._refuse('one_pass scoring', 'one_pass', over)
        if not 1 <= K <= 32:
            raise NotImplementedError('one_pass scoring takes seqs_per_image 1..32 (got %d)' % K)
        o = self._greedy_options(over)
        rows = int(B) * K
        pack_forced(caption_ids=caption_ids, rows=rows, max_length=o.max_length, last_tok=last_tok)      # the refusals only
        cap = torch.as_tensor(caption_ids).to(torch.int64).reshape(rows, o.max_length)
        lt = None if last_tok is None else torch.as_tensor(last_tok).to(torch.int64).reshape(rows)
        return o, cap, lt

    def _score_workspace(self, B, K, o, dev, slot):
        """The score workspace of a slot, cached like _workspace."""
        need = lib.vitcap_engine_score_workspace_bytes(B, K, C.byref(o))
        if need == 0:
            raise VitcapError('engine_score_workspace_bytes: %s' % lib.vitcap_last_error().decode())
        sws = self._score_ws.get(slot)
        if sws is None or sws.numel() < need or sws.device != dev:
            sws = torch.empty(need, dtype=torch.uint8, device=dev)
            self._score_ws[slot] = sws
        return sws, need

    def _score_one_pass(self, image, B, o, cap, lt, K, slot, dev, return_ids, maps=None, alts=None, vis=None):
        """One vitcap_engine_score_req call: `image` is encoded first, or with image None the slot's workspace holds the prefill.
        At most one of the three (vitcap_score_req.kind is a tag):
        vis = packed visibility words int32 (rows, 19) (vitcap_amd.occlusion.pack_visible): SCORE_MASKED; results as SCORE_PLAIN.
        maps = (per_head, layer_mask): SCORE_MAPS, -> (lp, tok_lp, ids, maps).
        alts = k: SCORE_ALTS, -> (lp, tok_lp, ids, Alternatives)."""
        rows = B * K
        ws, need = self._workspace(B, dev, slot, o)
        sws, sneed = self._score_workspace(B, K, o, dev, slot)
        lp = torch.empty((rows,), dtype=torch.float32, device=dev)
        tok_lp = torch.empty((rows, o.max_length), dtype=torch.float32, device=dev)
        ids = torch.empty((rows, 1, o.max_length), dtype=torch.int64, device=dev)
        req = L.score_req(B=B, opts=o, workspace=ws, workspace_bytes=need, caps_per_image=K, caption_ids=cap.to(dev).contiguous(),
                          last_tok=None if lt is None else lt.to(dev).contiguous(), score_ws=sws, score_ws_bytes=sneed,
                          out_logprobs=lp, out_token_logprobs=tok_lp, out_ids=ids)
        if image is not None:
            req.encode, req.image, req.image_is_bf16 = 1, image.data_ptr(), int(image.dtype == torch.bfloat16)
        extra = ()
        if maps is not None:
            per_head, layer_mask = maps
            W = 578 + o.max_length
            out = torch.zeros((rows, o.max_length, 4) + ((12, W) if per_head else (W,)), dtype=torch.float32, device=dev)
            req.kind, req.maps, req.per_head, req.layer_mask = L.SCORE_MAPS, out.data_ptr(), int(per_head), int(layer_mask)
            extra = (out,)
        elif alts is not None:
            from .alternatives import Alternatives
            k = int(alts)
            res = Alternatives(torch.empty((rows, o.max_length, k), dtype=torch.int32, device=dev),
                               torch.empty((rows, o.max_length, k), dtype=torch.float32, device=dev),
                               torch.empty((rows, o.max_length), dtype=torch.int32, device=dev),
                               torch.empty((rows, o.max_length), dtype=torch.float32, device=dev))      # the engine fills all of them
            req.kind, req.k = L.SCORE_ALTS, k
            req.alt_ids, req.alt_lp, req.rank, req.entropy = (x.data_ptr() for x in res)
            extra = (res,)
        elif vis is not None:
            # read in place by the enqueued kernels: allocated and released on this stream, so the block is not reused before them
            vis = vis.to(device=dev, dtype=torch.int32).contiguous()
            assert tuple(vis.shape) == (rows, 19)
            req.kind, req.vis_mask = L.SCORE_MASKED, vis.data_ptr()
        check(lib.vitcap_engine_score_req(self._engine, C.byref(req), _stream()), 'engine_score_req')
        if image is not None:
            self._encoded[slot] = (o, B)
        return (lp, tok_lp, ids) + extra if extra or return_ids else (lp, tok_lp)

    def _score_source(self, who, image, slot, caption_ids, K, last_tok, over, then=None):
        """The opening of every X / X_encoded pair: the host-side checks (_score_inputs), then `then(B)` -- checks of the caller that
        need the batch -- and only then the device.  image None: the images of the last run() / generate*() / score() call on
        `slot`, with the options laid out as that call's.  -> (image or None, B, opts, caption ids, last_tok or None, device)."""
        if image is not None:
            B = image.shape[0]
            o, cap, lt = self._score_inputs(B, caption_ids, K, last_tok, over)
        else:
            if slot not in self._encoded:
                raise RuntimeError('%s: no encoded images on slot %r (call run / generate / score on it first)' % (who, slot))
            self._refuse_patch_slot(who, slot)
            o_last, B = self._encoded[slot]
            o, cap, lt = self._score_inputs(B, caption_ids, K, last_tok, over)
            o.seqs_per_image = o_last.seqs_per_image      # the workspace of that call, as it was laid out
            if o.max_length != o_last.max_length or o_last.tag_visible > 0 or o_last.num_beams > 1 or o_last.use_cbs:
                raise ValueError('%s: the last call on slot %r ran other options (max_length / tags / beams)' % (who, slot))
        if then is not None:
            then(B)
        return image, B, o, cap, lt, (self._check_image(image) if image is not None else self._packed[2])

    def _greedy_caption(self, who, image, slot, over):
        """The opening of the caption_with_* calls: greedy captions only, then generate() through the staged path.
        -> (opts, ids, logprobs, last_tok)."""
        self._refuse(who, 'greedy', over)
        o = self._greedy_options(over)
        return (o,) + self.run(image, o, slot=slot, want_last=True)

    def score_encoded(self, caption_ids, seqs_per_image=1, slot=0, return_ids=False, last_tok=None, **over):
        """score(one_pass=True) against the images of the last run() / generate*() / score() call on `slot`, without encoding them again
        (a vitcap_score_req with encode = 0 reads the visual K/V that call left in the slot's workspace).  The options that size the
        workspace (max_length) must be those of that call."""
        K = int(seqs_per_image)
        image, B, o, cap, lt, dev = self._score_source('score_encoded', None, slot, caption_ids, K, last_tok, over)
        return self._score_one_pass(image, B, o, cap, lt, K, slot, dev, return_ids)

    @staticmethod
    def _layer_mask(layers):
        """(0, 1, 2, 3)-style selection of decoder layers -> the engine's bit mask."""
        ls = [int(l) for l in layers]
        if not ls or any(l < 0 or l > 3 for l in ls):
            raise ValueError('attention maps: layers must name at least one of the decoder layers 0..3 (got %r)' % (layers,))
        mask = 0
        for l in ls:
            mask |= 1 << l
        return mask

    def _attention_maps(self, who, image, caption_ids, seqs_per_image, per_head, layers, slot, last_tok, over):
        K, mask = int(seqs_per_image), self._layer_mask(layers)
        image, B, o, cap, lt, dev = self._score_source(who, image, slot, caption_ids, K, last_tok, over)
        lp, tok_lp, _, maps = self._score_one_pass(image, B, o, cap, lt, K, slot, dev, False, maps=(bool(per_head), mask))
        return lp, tok_lp, maps

    def attention_maps(self, image, caption_ids, seqs_per_image=1, per_head=False, layers=(0, 1, 2, 3), slot=0, last_tok=None, **over):
        """Where the model looked for each word of GIVEN captions: the softmax row of the [MASK] probe at every position t >= 1, in
        every selected decoder layer -- the reference's attention_probs[b, h, cur_len = t] (modeling_bert.py:320-342, 484-510) --
        from the one-pass scoring pass (a vitcap_score_req of kind VITCAP_SCORE_MAPS).  Inputs and refusals as score(one_pass=True).
        -> (logprobs (rows,), token_logprobs (rows, L), maps): maps fp32 (rows, L, 4, W), the mean over the 12 heads, or with
        per_head (rows, L, 4, 12, W); W = 578 + L, columns as vitcap_amd.attnmaps names them (0 tag cls, 1 encoder cls, 2..577 the
        24 x 24 patches, 578 + k token k, 578 + t the probe itself).  Position 0 and the positions behind a caption's first [SEP]
        are zeros; so are the layers not in `layers` (the engine leaves their slices untouched, the array starts zeroed)."""
        return self._attention_maps('attention_maps', image, caption_ids, seqs_per_image, per_head, layers, slot, last_tok, over)

    def attention_maps_encoded(self, caption_ids, seqs_per_image=1, per_head=False, layers=(0, 1, 2, 3), slot=0, last_tok=None, **over):
        """attention_maps() against the images of the last run() / generate*() / score() call on `slot`, without encoding them again
        (the request's encode = 0); the conditions of score_encoded()."""
        return self._attention_maps('attention_maps_encoded', None, caption_ids, seqs_per_image, per_head, layers, slot, last_tok, over)

    def caption_with_maps(self, image, per_head=False, layers=(0, 1, 2, 3), slot=0, **over):
        """Greedy captions and where the model looked for each of their words: generate() through the staged path, then
        attention_maps_encoded() on its own output (the token chosen at the last position handed over as last_tok).
        -> (ids (B, 1, L), logprobs (B, 1), maps)."""
        o, ids, lp, last = self._greedy_caption('caption_with_maps', image, slot, over)
        _, _, maps = self.attention_maps_encoded(ids.view(image.shape[0], o.max_length), 1, per_head=per_head, layers=layers, slot=slot,
                                                 last_tok=last, **over)
        return ids, lp, maps

    def _alternatives(self, who, image, caption_ids, seqs_per_image, k, slot, last_tok, over):
        from .alternatives import check_k
        K, k = int(seqs_per_image), check_k(k)
        image, B, o, cap, lt, dev = self._score_source(who, image, slot, caption_ids, K, last_tok, over)
        lp, tok_lp, _, alts = self._score_one_pass(image, B, o, cap, lt, K, slot, dev, False, alts=k)
        return lp, tok_lp, alts

    def alternatives(self, image, caption_ids, seqs_per_image=1, k=5, slot=0, last_tok=None, **over):
        """What the model would have said instead, at every position of GIVEN captions: from the logits of the one-pass scoring pass
        (a vitcap_score_req of kind VITCAP_SCORE_ALTS) the k best vocabulary entries per position with their log-probs, the rank of
        the scored word among all 30522 and the entropy of the position's distribution.  Inputs and refusals as score(one_pass=True);
        k is 1..16.
        -> (logprobs (rows,), token_logprobs (rows, L), alts): alts a vitcap_amd.alternatives.Alternatives of ids int32 (rows, L, k)
        best first (ties to the lower id), logprobs fp32 (rows, L, k), rank int32 (rows, L) (0 = the scored word is the first
        choice) and entropy fp32 (rows, L) in nats.  Position 0 and the positions behind a caption's first [SEP] hold ids = rank =
        -1 and logprobs = entropy = 0.  Where ids equals the scored word, logprobs equals token_logprobs bit for bit."""
        return self._alternatives('alternatives', image, caption_ids, seqs_per_image, k, slot, last_tok, over)

    def alternatives_encoded(self, caption_ids, seqs_per_image=1, k=5, slot=0, last_tok=None, **over):
        """alternatives() against the images of the last run() / generate*() / score() call on `slot`, without encoding them again
        (the request's encode = 0); the conditions of score_encoded()."""
        return self._alternatives('alternatives_encoded', None, caption_ids, seqs_per_image, k, slot, last_tok, over)

    def caption_with_alternatives(self, image, k=5, slot=0, want_token_logprobs=False, **over):
        """Greedy captions and, for each of their words, what else the model could have said: generate() through the staged path,
        then alternatives_encoded() on its own output (the token chosen at the last position handed over as last_tok).
        The alternatives are those of the ONE-PASS pass, which rounds differently from the step loop that chose the words: the
        chosen word is therefore usually, but not always, rank 0, and its log-prob among the alternatives differs from the caption's
        own in the last bits.  -> (ids (B, 1, L), logprobs (B, 1), alts); with want_token_logprobs the one-pass pass's per-token
        log-probs of the caption's words (B, L) come last."""
        from .alternatives import check_k
        k = check_k(k)
        o, ids, lp, last = self._greedy_caption('caption_with_alternatives', image, slot, over)
        _, tok_lp, alts = self.alternatives_encoded(ids.view(image.shape[0], o.max_length), 1, k=k, slot=slot, last_tok=last, **over)
        return (ids, lp, alts, tok_lp) if want_token_logprobs else (ids, lp, alts)

    # ---- occlusion: given captions scored with visual keys hidden from them (vitcap_score_req of kind VITCAP_SCORE_MASKED)
    def _score_masked(self, who, image, caption_ids, visible, seqs_per_image, slot, return_ids, last_tok, over):
        from .occlusion import as_visible, pack_visible
        K, vis = int(seqs_per_image), []
        image, B, o, cap, lt, dev = self._score_source(who, image, slot, caption_ids, K, last_tok, over,
                                                       then=lambda B: vis.append(pack_visible(as_visible(visible, B * K))))
        return self._score_one_pass(image, B, o, cap, lt, K, slot, dev, return_ids, vis=vis[0])

    def score_masked(self, image, caption_ids, visible, seqs_per_image=1, slot=0, return_ids=False, last_tok=None, one_pass=True, **over):
        """score(one_pass=True) with visual keys hidden from the captions: `visible`, bool or uint8, one row per caption, either
        (rows, 578) in the cache's order (0 tag cls, 1 encoder cls, 2..577 the 24 x 24 patches row-major) or a (rows, 24, 24) patch
        grid (both cls columns then stay visible); nonzero = the caption's rows may attend that visual token, in all four decoder
        layers -- the reference's attention_mask zeros on caption rows / visual columns (modeling_bert.py:1498-1501).  The mask hides
        visual TOKENS from the CAPTION; the encoder and the prefill still see the whole image.  Inputs and refusals as
        score(one_pass=True); a wrong shape or dtype of `visible` is a ValueError before the GPU is touched.  With everything visible
        the results are score(one_pass=True)'s, bit for bit.
        one_pass=False: the same captions and masks through the masked step loop (vitcap_engine_generate_masked with forced tokens),
        the stepwise counterpart score() has; seqs_per_image 1..8; with everything visible the results are score()'s, bit for bit."""
        if not one_pass:
            from .forced import pack_forced
            from .occlusion import as_visible, pack_visible
            self.refuse_visible('score_masked', over)
            K = int(seqs_per_image)
            o = self.gen_options(num_beams=1, do_sample=False, num_return_sequences=1, num_keep_best=1, **dict(over, use_graph=False))
            o.seqs_per_image = K
            check(lib.vitcap_gen_opts_check(C.byref(o)), 'gen_opts')
            rows = image.shape[0] * K
            vis = pack_visible(as_visible(visible, rows))
            forced, sf = pack_forced(caption_ids=caption_ids, rows=rows, max_length=o.max_length, last_tok=last_tok)
            ids, lp, tok_lp = self.run(image, o, slot=slot, forced=forced, score_forced=sf, want_token_logprobs=True, vis=vis)
            return (lp.view(-1), tok_lp, ids) if return_ids else (lp.view(-1), tok_lp)
        return self._score_masked('score_masked', image, caption_ids, visible, seqs_per_image, slot, return_ids, last_tok, over)

    def score_masked_encoded(self, caption_ids, visible, seqs_per_image=1, slot=0, return_ids=False, last_tok=None, **over):
        """score_masked() against the images of the last run() / generate*() / score() call on `slot`, without encoding them again
        (the request's encode = 0); the conditions of score_encoded()."""
        return self._score_masked('score_masked_encoded', None, caption_ids, visible, seqs_per_image, slot, return_ids, last_tok, over)

    def _score_variants(self, image, B, o, cap, lt, masks, slot, dev):
        """Every caption of cap (B * K, L) under every mask row of `masks` bool (V, 578), in passes of at most 32 variants per image
        (K * variants <= 32 rows per image and pass); the first pass encodes when an image is given, the later ones read its prefill.
        -> (logprobs (B * K, V), token_logprobs (B * K, V, L))."""
        from .occlusion import MAX_ROWS, pack_visible
        K, V, L = cap.shape[0] // B, masks.shape[0], cap.shape[1]
        words = pack_visible(masks)                                    # (V, 19)
        per = max(1, MAX_ROWS // K)
        lps, toks = [], []
        for v0 in range(0, V, per):
            n = min(per, V - v0)
            c = cap.repeat_interleave(n, 0)                            # caption-major: the n variants of a caption are adjacent
            t = None if lt is None else lt.repeat_interleave(n, 0)
            w = words[v0:v0 + n].repeat(B * K, 1)
            lp, tok = self._score_one_pass(image if v0 == 0 else None, B, o, c, t, K * n, slot, dev, False, vis=w)
            lps.append(lp.view(B * K, n))
            toks.append(tok.view(B * K, n, L))
        return torch.cat(lps, 1), torch.cat(toks, 1)

    def _occlusion_maps(self, who, image, caption_ids, window, stride, keep_cls, keep_only, slot, last_tok, over):
        from .occlusion import check_window, window_masks
        window, stride, g = check_window(window, stride)
        image, B, o, cap, lt, dev = self._score_source(who, image, slot, caption_ids, 1, last_tok, over)
        masks = torch.cat([torch.ones((1, 578), dtype=torch.bool), window_masks(window, stride, keep_cls, keep_only)], 0)
        lp, tok = self._score_variants(image, B, o, cap, lt, masks, slot, dev)
        drop = tok[:, :1] - tok[:, 1:]                                 # (B, G, L)
        return lp[:, 0], tok[:, 0], drop.permute(0, 2, 1).reshape(B, cap.shape[1], g, g)

    def occlusion_maps(self, image, caption_ids, window=4, stride=None, keep_cls=True, keep_only=False, slot=0, last_tok=None, **over):
        """How much less likely each word of a GIVEN caption becomes when the caption cannot see a region of the image: the caption
        (one per image, caption_ids (B, L)) is scored unoccluded and once per window position -- a window x window block of the
        24 x 24 patch grid hidden from it (with keep_only: everything BUT the block hidden), windows `stride` apart (default: window;
        (24 - window) % stride must be 0).  keep_cls: the two cls tokens (columns 0, 1) stay visible in the occluded variants.  The
        variants of an image share its encoder pass and visual K/V, 32 per scoring pass (score_masked).
        -> (logprobs (B,), token_logprobs (B, L): the unoccluded scores, and drop (B, L, gh, gw)):
        drop[b, t, i, j] = token_logprobs[b, t] - the same with window (i, j) hidden; gh = gw = (24 - window) / stride + 1; zero at
        position 0 and behind the caption's end, where both terms are.  Occlusion hides visual tokens from the caption only: the
        encoder has seen the whole image.  Inputs and refusals as score(one_pass=True)."""
        return self._occlusion_maps('occlusion_maps', image, caption_ids, window, stride, keep_cls, keep_only, slot, last_tok, over)

    def occlusion_maps_encoded(self, caption_ids, window=4, stride=None, keep_cls=True, keep_only=False, slot=0, last_tok=None, **over):
        """occlusion_maps() against the images of the last run() / generate*() / score() call on `slot`, without encoding them again;
        the conditions of score_encoded()."""
        return self._occlusion_maps('occlusion_maps_encoded', None, caption_ids, window, stride, keep_cls, keep_only, slot, last_tok, over)

    def caption_with_occlusion(self, image, window=4, stride=None, keep_cls=True, keep_only=False, slot=0, **over):
        """Greedy captions and the occlusion maps of their words: generate() through the staged path, then occlusion_maps_encoded()
        on its own output (the token chosen at the last position handed over as last_tok).  -> (ids (B, 1, L), logprobs (B, 1),
        drop (B, L, gh, gw))."""
        from .occlusion import check_window
        check_window(window, stride)
        o, ids, lp, last = self._greedy_caption('caption_with_occlusion', image, slot, over)
        _, _, drop = self.occlusion_maps_encoded(ids.view(image.shape[0], o.max_length), window, stride, keep_cls, keep_only, slot=slot,
                                                 last_tok=last, **over)
        return ids, lp, drop

    def visual_gain(self, image, caption_ids, seqs_per_image=1, slot=0, last_tok=None, **over):
        """What the image added to each word of GIVEN captions: token_logprobs minus the token_logprobs with all 578 visual keys
        hidden from the caption (it then attends its own tokens only), from two variants per caption.  Inputs and refusals as
        score(one_pass=True).  -> fp32 (rows, L), zero at position 0 and behind a caption's end."""
        image, B, o, cap, lt, dev = self._score_source('visual_gain', image, slot, caption_ids, int(seqs_per_image), last_tok, over)
        masks = torch.stack([torch.ones(578, dtype=torch.bool), torch.zeros(578, dtype=torch.bool)])
        _, tok = self._score_variants(image, B, o, cap, lt, masks, slot, dev)
        return tok[:, 0] - tok[:, 1]

    # ---- region captions: captions the model writes with everything outside a region hidden from them (vitcap_engine_*_masked)
    def _caption_regions(self, who, image, regions, keep_cls, slot, over):
        from .occlusion import pack_visible
        from .regions import MAX_REGIONS, region_masks
        self._refuse(who, 'regions', over)
        if image is not None:
            B = image.shape[0]
        else:
            if slot not in self._encoded:
                raise RuntimeError('%s: no encoded images on slot %r (call run / generate / score on it first)' % (who, slot))
            B = self._encoded[slot][1]
        masks, _ = region_masks(regions, B, keep_cls)                  # (B, R, 578)
        R = masks.shape[1]
        o = self._greedy_options(over, no_graph=True)
        all_ids, all_lp = [], []
        for r0 in range(0, R, MAX_REGIONS):
            n = min(MAX_REGIONS, R - r0)
            ok = type(o).from_buffer_copy(o)
            ok.seqs_per_image = n
            check(lib.vitcap_gen_opts_check(C.byref(ok)), 'gen_opts')
            vis = pack_visible(masks[:, r0:r0 + n].reshape(B * n, -1))
            # the first pass encodes; the later ones decode on its prefill
            ids, lp = self.run(image if r0 == 0 else None, ok, slot=slot, vis=vis)
            all_ids.append(ids.view(B, n, ok.max_length))
            all_lp.append(lp.view(B, n))
        return torch.cat(all_ids, 1), torch.cat(all_lp, 1)

    def caption_regions(self, image, regions, keep_cls=True, slot=0, **over):
        """One greedy caption per region of every image, everything outside the region hidden from that caption (generate(visible=)
        with the region's mask).  regions: integer boxes (B, R, 4) or (R, 4) -- the same for every image -- as [row0, col0, row1,
        col1), half-open, on the 24 x 24 patch grid, or bool grids (B, R, 24, 24) (vitcap_amd.regions; grid_regions(g) gives the
        g x g tiling).  keep_cls: the two cls tokens stay visible to every caption.  Any R: the image is encoded once, its regions are
        decoded in passes of up to 8 sequences per image that share its visual K/V.  The mask hides visual TOKENS from the caption; a
        hidden patch has still shaped its neighbours and the cls tokens inside the encoder.  Bad boxes are a ValueError, beams / CBS /
        visible tags / sampling a NotImplementedError, before the GPU is touched.
        -> (ids (B, R, L), logprobs (B, R)); each equal to generate(image, visible=region mask)'s, bit for bit, while the decode
        step takes the same GEMM forms (B * 8 <= 128 sequences)."""
        return self._caption_regions('caption_regions', image, regions, keep_cls, slot, over)

    def caption_regions_encoded(self, regions, keep_cls=True, slot=0, **over):
        """caption_regions() against the images of the last run() / generate*() / score() call on `slot`, without encoding them
        again (vitcap_engine_decode_masked on that call's prefill); max_length must be that call's, and it ran without visible tags."""
        return self._caption_regions('caption_regions_encoded', None, regions, keep_cls, slot, over)

    def caption_with_regions(self, image, regions, keep_cls=True, slot=0, **over):
        """Greedy captions of the whole images and of their regions on one encoder pass: generate() through the staged path, then
        caption_regions_encoded().  -> (ids (B, 1, L), logprobs (B, 1), region ids (B, R, L), region logprobs (B, R))."""
        from .regions import region_masks
        self.refuse_visible('caption_with_regions', over)
        region_masks(regions, image.shape[0], keep_cls)      # the refusals, before the GPU is touched
        o, ids, lp, _ = self._greedy_caption('caption_with_regions', image, slot, over)
        rids, rlp = self.caption_regions_encoded(regions, keep_cls=keep_cls, slot=slot, **over)
        return ids, lp, rids, rlp

    def generate_beam(self, image, num_beams, length_penalty=1.0, slot=0, num_keep_best=1, visible=None, keep_cls=True, **over):
        """Beam search -> (ids (B,num_keep_best,L), logprobs (B,num_keep_best)), best hypothesis first, like
        ViTCAP._generate_beam_search (modeling_utils.py:888-1100).
        visible: as generate() takes it, one row per image -- (B, 578) in cache order or a (B, 24, 24) patch grid (the two cls columns
        then visible iff keep_cls): all beams of an image are searched with the other visual tokens hidden from them
        (vitcap_engine_generate_beam_masked).  Then num_beams 2..8; num_beams == 1, CBS, visible tags, beam sampling, hipGraph replay
        and forced tokens are a NotImplementedError naming the option, a bad mask a ValueError, before the GPU is touched."""
        if visible is not None:
            from .occlusion import as_visible, pack_visible
            self.refuse_visible_beam('generate_beam', num_beams, over)
            vis = pack_visible(as_visible(visible, image.shape[0], keep_cls))
            o = self._beam_masked_options(num_beams, length_penalty, num_keep_best, over)
            return self._run_beam_masked(image, o, [vis], slot)[0]
        over.setdefault('do_sample', False)      # do_sample=True: beam sampling (modeling_utils.py:966-985), temperature / top_k / top_p / seed
        o = self.gen_options(num_beams=int(num_beams), length_penalty=float(length_penalty), num_keep_best=int(num_keep_best),
                             num_return_sequences=1, **over)
        return self.run(image, o, slot=slot)

    # ---- region captions under beam search (vitcap_engine_*_beam_masked): one mask row per image, all its beams see the same part
    def refuse_visible_beam(self, who, num_beams, over=None):
        """What a visibility mask under beam search is not built for, refused by the option's name before the GPU is touched."""
        if isinstance(num_beams, bool) or int(num_beams) != num_beams or not 2 <= int(num_beams) <= 8:
            raise NotImplementedError('%s: a visibility mask under beam search needs num_beams 2..8 (got num_beams=%r; one beam is '
                                      'generate(visible=) / caption_regions)' % (who, num_beams))
        te = self._refuse(who, 'visible_beam', over)
        for k in self._FORCED_KEYS:
            if te.get(k) is not None and te.get(k) is not False:
                raise NotImplementedError('%s: %s -- forced tokens under beam search are not built' % (who, k))

    _FORCED_KEYS = ('prefix_ids', 'forced_ids', 'want_token_logprobs')

    def _beam_masked_options(self, num_beams, length_penalty, num_keep_best, over):
        return self._greedy_options(over, no_graph=True, drop=self._FORCED_KEYS, num_beams=int(num_beams),
                                    length_penalty=float(length_penalty), num_keep_best=int(num_keep_best))

    def _run_beam_masked(self, image, opts, vis_list, slot, whole=False):
        """The images are encoded and prefilled once under the beam options `opts`; then, with `whole`, one plain beam decode, and one
        vitcap_engine_decode_beam_masked pass per packed mask (B, 19) of vis_list on that prefill.  A single mask without `whole` is
        one vitcap_engine_generate_beam_masked call.  -> [(ids (B, keep, L), logprobs (B, keep)), ...], the whole-image result first."""
        dev, B = self._check_image(image), image.shape[0]
        for v in vis_list:
            if tuple(v.shape) != (B, 19):
                raise ValueError('the packed visibility mask must be (%d, 19), got %s' % (B, tuple(v.shape)))
        # read in place by the enqueued kernels: allocated and released on this stream, so the blocks are not reused before them
        vis_list = [v.to(device=dev, dtype=torch.int32).contiguous() for v in vis_list]
        ws, need = self._workspace(B, dev, slot, opts)
        self._encoded[slot] = (opts, B)
        self._last = (slot, opts, B)
        if len(vis_list) == 1 and not whole:
            ids, lp = self._out_buffers(B, opts, dev)
            self._decode('beam_masked', image, B, opts, ws, need, ids, lp, (None, None), vis=vis_list[0])
            return [(ids, lp)]
        self._encode_prefill(image, opts, ws, need, _stream())
        out = []
        for v in ([None] if whole else []) + vis_list:      # None: the plain beam decode of the whole image
            ids, lp = self._out_buffers(B, opts, dev)
            self._decode('' if v is None else 'beam_masked', None, B, opts, ws, need, ids, lp, (None,), vis=v)
            out.append((ids, lp))
        return out

    def _caption_regions_beam(self, who, image, regions, num_beams, num_keep_best, length_penalty, keep_cls, slot, over, whole):
        from .occlusion import pack_visible
        from .regions import region_masks
        self.refuse_visible_beam(who, num_beams, over)
        B = image.shape[0]
        masks, _ = region_masks(regions, B, keep_cls)                  # (B, R, 578)
        R = masks.shape[1]
        o = self._beam_masked_options(num_beams, length_penalty, num_keep_best, over)
        res = self._run_beam_masked(image, o, [pack_visible(masks[:, r]) for r in range(R)], slot, whole=whole)
        reg = res[1:] if whole else res
        rids, rlp = torch.stack([x[0] for x in reg], 1), torch.stack([x[1] for x in reg], 1)
        return (res[0][0], res[0][1], rids, rlp) if whole else (rids, rlp)

    def caption_regions_beam(self, image, regions, num_beams, num_keep_best=1, length_penalty=1.0, keep_cls=True, slot=0, **over):
        """caption_regions() by beam search: per region of every image its num_keep_best best captions under num_beams beams (2..8),
        everything outside the region hidden from all beams (generate_beam(visible=) with the region's mask).  regions / keep_cls: as
        caption_regions().  The images are encoded and prefilled once under the beam options; every region index is one
        vitcap_engine_decode_beam_masked pass on that prefill.  Bad boxes are a ValueError; num_beams == 1, CBS, visible tags, sampling,
        use_graph and forced tokens a NotImplementedError naming the option, before the GPU is touched.
        -> (ids (B, R, num_keep_best, L), logprobs (B, R, num_keep_best)), best first."""
        return self._caption_regions_beam('caption_regions_beam', image, regions, num_beams, num_keep_best, length_penalty, keep_cls, slot,
                                          over, False)

    def caption_with_regions_beam(self, image, regions, num_beams, num_keep_best=1, length_penalty=1.0, keep_cls=True, slot=0, **over):
        """The whole-image beam captions and the region captions of caption_regions_beam() on one encoder pass: generate_beam(image,
        num_beams, ...) through the staged path, then the region passes on its prefill.
        -> (ids (B, keep, L), logprobs (B, keep), region ids (B, R, keep, L), region logprobs (B, R, keep))."""
        return self._caption_regions_beam('caption_with_regions_beam', image, regions, num_beams, num_keep_best, length_penalty, keep_cls,
                                          slot, over, True)

    # ---- patch removal: tags, captions and scores of an image with patches taken out of EVERY attention row of the model
    # (vitcap_engine_encode_patches / vitcap_engine_prefill_patches, then the `_masked` calls with the same words)
    def _refuse_patch_slot(self, who, slot):
        """The `*_encoded` calls carry no presence mask: on a slot that holds a patch-removed encoding they would let the caption
        rows see the removed patches' rows."""
        if isinstance(self._encoded.get(slot), _PatchEncoded):
            raise RuntimeError('%s: slot %r holds a patch-removed encoding (tag_patches / caption_patches / score_patches / caption_crops); '
                               'this call carries no presence mask, so the removed patches would be visible to it -- encode the images '
                               'again, or use the *_patches calls' % (who, slot))

    def refuse_patches(self, who, over=None):
        """Patch removal exists for the greedy loop and the one-pass scorer without visible tags and without a hipGraph: anything else
        is refused by the option's name, before the GPU is touched."""
        self._refuse(who, 'patches', over)

    def _encode_patches(self, image, words, o, slot):
        """Encoder and prefill of `image` under the packed presence rows `words` (B, 19) -> (workspace, bytes, words on the device)."""
        dev, B = self._check_image(image), image.shape[0]
        if tuple(words.shape) != (B, 19):
            raise ValueError('the packed presence mask must be (%d, 19), got %s' % (B, tuple(words.shape)))
        # read in place by the enqueued kernels: allocated and released on this stream, so the block is not reused before them
        words = words.to(device=dev, dtype=torch.int32).contiguous()
        ws, need = self._workspace(B, dev, slot, o)
        check(lib.vitcap_engine_encode_patches(*self._head(image, B, o, ws, need), _p(words), _stream()), 'engine_encode_patches')
        check(lib.vitcap_engine_prefill_patches(*self._head(None, B, o, ws, need), _p(words), _stream()), 'engine_prefill_patches')
        enc = _PatchEncoded((o, B))
        enc.words = words
        self._encoded[slot] = enc
        self._last = (slot, o, B)
        return ws, need, words

    def _tags_of_slot(self, o, B, ws, slot):
        """(tag_logits (B, 30522), tag_topk (B, 50), tag_prob (B, 50), tag_len (B,)) of the encoding on `slot`."""
        dev = ws.device
        logits = torch.empty((B, L.VOCAB), dtype=torch.float32, device=dev)
        topk = torch.empty((B, 50), dtype=torch.int64, device=dev)
        check(lib.vitcap_engine_tags(self._engine, B, C.byref(o), _p(ws), _p(logits), _p(topk), _stream()), 'engine_tags')
        return (logits, topk, self.tap('tag_prob', B, (B, 50), slot=slot, opts=o),
                self.tap('tag_len', B, (B,), dtype=torch.int64, slot=slot, opts=o))

    def tag_patches(self, image, present, slot=0, **over):
        """The concept tagger on the images without their absent patches: `present` is a (B, 24, 24) or (B, 576) bool (row-major
        patch grid; the two cls keys are always present), and an absent patch is removed as a key from every attention row of all
        12 + 4 ViT blocks -- the reference's additive ViT mask with -10000 in that column (modeling_bert.py:458-478).  Runs the encoder
        (and the prefill) only and leaves the slot encoded for the other *_patches calls.
        -> (tag_logits (B, 30522), tag_topk (B, 50), tag_prob (B, 50), tag_len (B,))."""
        from .patches import pack_present
        self.refuse_patches('tag_patches', over)
        o = self._greedy_options(over, no_graph=True)
        words = pack_present(present, image.shape[0])
        ws, _, _ = self._encode_patches(image, words, o, slot)
        return self._tags_of_slot(o, image.shape[0], ws, slot)

    def caption_patches(self, image, present, want_tags=False, want_token_logprobs=False, slot=0, **over):
        """The greedy caption of the images without their absent patches (`present` as tag_patches takes it): the encoder, the
        decoder's visual rows and the caption rows all run without those keys, which is the reference with the column at -10000 in the
        ViT mask and at 0 in attention_mask.  With every patch present the result is generate()'s, bit for bit.
        -> (ids (B, 1, L), logprobs (B, 1)) [+ token_logprobs (B, L)]; with want_tags, self.last_tags = (tag_logits, tag_topk) and
        self.last_tag_probs = (tag_prob, tag_len).  CBS, beams, visible tags, use_graph and sampling are a NotImplementedError."""
        from .patches import pack_present
        self.refuse_patches('caption_patches', over)
        o = self._greedy_options(over, no_graph=True)
        B = image.shape[0]
        words = pack_present(present, B)
        ws, need, words = self._encode_patches(image, words, o, slot)
        if want_tags:
            tags = self._tags_of_slot(o, B, ws, slot)
            self.last_tags, self.last_tag_probs = tags[:2], tags[2:]
        ids, lp = self._out_buffers(B, o, ws.device)
        tok_lp = torch.empty((B, o.max_length), dtype=torch.float32, device=ws.device) if want_token_logprobs else None
        self._decode('masked', None, B, o, ws, need, ids, lp, (None,), tok_lp=tok_lp, vis=words)
        return (ids, lp, tok_lp) if want_token_logprobs else (ids, lp)

    def score_patches(self, image, caption_ids, present, seqs_per_image=1, slot=0, return_ids=False, last_tok=None, **over):
        """score(one_pass=True) of GIVEN captions on the images without their absent patches: encoder and prefill under `present`
        (one row per image), then the one-pass scorer with the same words hidden from every caption of the image (VITCAP_SCORE_MASKED).
        -> (logprob (rows,), token_logprobs (rows, L)); with return_ids also the ids."""
        from .patches import pack_present
        K = int(seqs_per_image)
        B = image.shape[0]
        self.refuse_patches('score_patches', over)
        words = pack_present(present, B)
        o, cap, lt = self._score_inputs(B, caption_ids, K, last_tok, dict(over, use_graph=False))
        _, _, words = self._encode_patches(image, words, o, slot)
        return self._score_one_pass(None, B, o, cap, lt, K, slot, self._packed[2], return_ids, vis=words.repeat_interleave(K, 0))

    def caption_crops(self, image, regions, slot=0, **over):
        """Tags and greedy caption of every region of every image SEEN ALONE: each (image, region) pair is encoded as an image of its
        own with every patch outside the region removed (caption_patches with the region as `present`).  regions: as caption_regions
        takes them.  The pairs are encoded in passes of up to patches.MAX_CROPS; each pass gathers its own images.
        -> (ids (B, R, L), logprobs (B, R), tag_topk (B, R, 50), tag_prob (B, R, 50))."""
        from .patches import MAX_CROPS, crop_masks
        self.refuse_patches('caption_crops', over)
        B = image.shape[0]
        present, _ = crop_masks(regions, B)                   # (B, R, 24, 24)
        R = present.shape[1]
        self._check_image(image)
        pair_b = torch.arange(B).repeat_interleave(R)
        pair_r = torch.arange(R).repeat(B)
        out = [[], [], [], []]
        for p0 in range(0, B * R, MAX_CROPS):
            pb, pr = pair_b[p0:p0 + MAX_CROPS], pair_r[p0:p0 + MAX_CROPS]
            ids, lp = self.caption_patches(image.index_select(0, pb.to(image.device)), present[pb, pr], want_tags=True, slot=slot, **over)
            for dst, x in zip(out, (ids[:, 0], lp[:, 0], self.last_tags[1], self.last_tag_probs[0])):
                dst.append(x)
        ids, lp, topk, prob = (torch.cat(x, 0) for x in out)
        return ids.view(B, R, -1), lp.view(B, R), topk.view(B, R, 50), prob.view(B, R, 50)

    def caption_with_crops(self, image, regions, slot=0, **over):
        """The whole-image greedy caption and tags, then caption_crops().
        -> (ids (B, 1, L), logprobs (B, 1), tag_topk (B, 50), tag_prob (B, 50), crop ids (B, R, L), crop logprobs (B, R),
            crop tag_topk (B, R, 50), crop tag_prob (B, R, 50))."""
        from .patches import crop_masks
        self.refuse_patches('caption_with_crops', over)
        B = image.shape[0]
        crop_masks(regions, B)                                # the refusals, before the GPU is touched
        ids, lp = self.caption_patches(image, torch.ones((B, 24, 24), dtype=torch.bool), want_tags=True, slot=slot, **over)
        topk, prob = self.last_tags[1], self.last_tag_probs[0]
        return (ids, lp, topk, prob) + self.caption_crops(image, regions, slot=slot, **over)

    # ---- encoder attention rollout: the ViT blocks' attention written out (vitcap_engine_encode_maps) and composed over the model's
    # graph (vitcap_amd.rollout.rollout_rows), for the tag head's CLS and for every word of a caption
    def refuse_rollout(self, who, over=None):
        """The encoder's attention is written out by a plain greedy / one-pass pass without visible tags and without a hipGraph:
        anything else is refused by the option's name, before the GPU is touched."""
        self._refuse(who, 'rollout', over)

    def _rollout_options(self, who, slot, over):
        """The refusals, then -> the validated options of a greedy pass without a hipGraph."""
        self.refuse_rollout(who, over)
        self._refuse_patch_slot(who, slot)
        return self._greedy_options(over, no_graph=True)

    def _encode_maps(self, image, o, slot, mask, per_head):
        """vitcap_engine_encode_maps + vitcap_engine_prefill of `image` on `slot` -> (maps (n_sel, B, [12,] 577, 577), workspace,
        bytes).  The slot is left encoded, as by run()."""
        dev, B = self._check_image(image), image.shape[0]
        n_sel = bin(mask).count('1')
        maps = torch.empty((n_sel, B) + ((12,) if per_head else ()) + (577, 577), dtype=torch.float32, device=dev)
        ws, need = self._workspace(B, dev, slot, o)
        check(lib.vitcap_engine_encode_maps(*self._head(image, B, o, ws, need), mask, int(bool(per_head)), _p(maps), maps.numel() * 4,
                                            _stream()), 'engine_encode_maps')
        check(lib.vitcap_engine_prefill(*self._head(None, B, o, ws, need), _stream()), 'engine_prefill')
        self._encoded[slot] = (o, B)
        self._last = (slot, o, B)
        return maps, ws, need

    @staticmethod
    def _image_chunks(image, n_sel, per_head):
        from . import rollout as R
        n = R.images_per_call(n_sel, per_head, R.MAX_CALL_BYTES)
        return [image[i:i + n] for i in range(0, image.shape[0], n)]

    def encoder_attention(self, image, blocks=None, per_head=False, slot=0, **over):
        """The attention matrices of the ViT blocks: the reference's `attn` of Attention.forward after its softmax
        (vision_transformer.py:179-183), written out by the encoder pass itself (vitcap_engine_encode_maps).  blocks: None (all 16)
        or ints 0..15 / names 'blocks.3', 'tag_blocks.0' (12..15 are the tag blocks).
        -> (maps fp32 (n_sel, B, 577, 577), the mean over the 12 heads, or with per_head (n_sel, B, 12, 577, 577); the names of the
        selected blocks, ascending).  Rows and columns are the encoder's tokens [cls | 576 patches]; the last tag block holds its cls
        row only (the pooler reads nothing else), zeros below.  The images are cut into chunks so that one engine call's buffer stays
        at or below 1 GiB (head mean, all blocks: 21.3 MB per image; per head: 256 MB).  There is no *_encoded form: the matrices are
        not kept on the workspace."""
        from . import rollout as R
        mask, names = R.parse_blocks(blocks)
        o = self._rollout_options('encoder_attention', slot, over)
        parts = [self._encode_maps(img, o, slot, mask, per_head)[0] for img in self._image_chunks(image, len(names), per_head)]
        return (parts[0] if len(parts) == 1 else torch.cat(parts, 1)), names

    def tag_rollout(self, image, residual=0.5, slot=0, **over):
        """Where the concept tagger looked: attention rollout (vitcap_amd.rollout) of the token the tag head's pooler reads --
        tag_hidden[:, 0], modeling_bert.py:1424 -- back through tag blocks 3..0 and blocks 7..0 to the image patches.  Rollout is a
        model of information flow through attention alone (head-mean attention mixed with `residual` of the identity per block); the
        MLPs and value vectors play no part in it.
        -> (patches (B, 24, 24), cls_mass (B,), tag_ids (B, 50), tag_prob (B, 50), tag_len (B,)): patches.sum + cls_mass = 1 per image;
        the tags are those of the same encoder pass.  No *_encoded form: the matrices are not kept on the workspace."""
        from . import rollout as R
        r = R.check_residual(residual)
        o = self._rollout_options('tag_rollout', slot, over)
        out = []
        for img in self._image_chunks(image, R.N_BLOCKS, False):
            A, ws, _ = self._encode_maps(img, o, slot, R.ALL_BLOCKS, False)
            _, topk, prob, tlen = self._tags_of_slot(o, img.shape[0], ws, slot)
            w = torch.zeros((img.shape[0], 1, R.N_VIS), dtype=torch.float32, device=A.device)
            w[..., 0] = 1.0
            grid, cls = R.patch_grid(R.rollout_rows(A, w, r)[:, 0])
            out.append((grid, cls, topk, prob, tlen))
        return tuple(torch.cat(x, 0) for x in zip(*out))

    def _rollout_chunk(self, img, o, cap, lt, K, lmask, nl, r, slot, want_tag=False):
        """One chunk of rollout_maps: encoder with maps, prefill, the maps form of the one-pass scorer on the same workspace, the
        rollout of every probe row.  cap None: the chunk's own greedy captions (K = 1), decoded first.  want_tag: the tag head's map
        (tag_rollout's, w = e_0) from the same matrices.
        -> (lp, tok_lp, patches, cls_mass, text_mass[, ids, caption logprobs][, tag patches (B, 24, 24), tag cls_mass (B,)])."""
        from . import rollout as R
        B, Lm = img.shape[0], o.max_length
        A, ws, need = self._encode_maps(img, o, slot, R.ALL_BLOCKS, False)
        own = ()
        if cap is None:
            ids, glp = self._out_buffers(B, o, A.device)
            lt = torch.empty((B,), dtype=torch.int64, device=A.device)
            self._decode('', None, B, o, ws, need, ids, glp, (lt,))
            cap, own = ids.view(B, Lm), (ids, glp)
        lp, tok_lp, _, maps = self._score_one_pass(None, B, o, cap, lt, K, slot, A.device, False, maps=(False, lmask))
        m = maps.view(B, K, Lm, 4, maps.shape[-1]).sum(3) * (1.0 / nl)      # unselected layers are zeros; NOT renormalised
        text = m[..., R.N_VIS:].sum(-1)
        v = torch.stack([R.rollout_rows(A, m[:, k, :, :R.N_VIS].contiguous(), r) for k in range(K)], 1)      # (B, K, L, 577)
        grid, cls = R.patch_grid(v.view(B * K, Lm, R.N_ENC))
        if want_tag:
            w = torch.zeros((B, 1, R.N_VIS), dtype=torch.float32, device=A.device)
            w[..., 0] = 1.0
            own = own + R.patch_grid(R.rollout_rows(A, w, r)[:, 0])
        return (lp, tok_lp, grid, cls, text.reshape(B * K, Lm)) + own

    def rollout_maps(self, image, caption_ids, seqs_per_image=1, layers=(0, 1, 2, 3), residual=0.5, slot=0, last_tok=None, **over):
        """Where each word of GIVEN captions looked, on the image's patches: the head-mean probe row of attention_maps() over the 578
        visual tokens, averaged over the selected decoder layers and NOT renormalised, carried back through the encoder by attention
        rollout (vitcap_amd.rollout.rollout_rows: the caption's visual tokens through blocks 11..8, the tag-branch cls through the tag
        blocks, both through blocks 7..0).  Inputs and refusals as score(one_pass=True); one encoder pass per chunk of images.
        What the maps are: a model of information flow through attention alone.  The decoder's own visual-to-visual mixing (its 4
        layers also update the visual rows) is not rolled; with layers=(0,) the visual keys are the raw encoder outputs and nothing
        is left out.
        -> (logprobs (rows,), token_logprobs (rows, L), patches (rows, L, 24, 24), cls_mass (rows, L), text_mass (rows, L)), the
        scores those of score(one_pass=True); patches.sum + cls_mass + text_mass = 1 at every live position, dead positions are 0.
        No *_encoded form: the matrices are not kept on the workspace."""
        from . import rollout as R
        r, K, lmask = R.check_residual(residual), int(seqs_per_image), self._layer_mask(layers)
        nl = bin(lmask).count('1')
        self.refuse_rollout('rollout_maps', over)
        self._refuse_patch_slot('rollout_maps', slot)
        o, cap, lt = self._score_inputs(image.shape[0], caption_ids, K, last_tok, dict(over, use_graph=False))
        out, i = [], 0
        for img in self._image_chunks(image, R.N_BLOCKS, False):
            n = img.shape[0]
            out.append(self._rollout_chunk(img, o, cap[i * K:(i + n) * K], None if lt is None else lt[i * K:(i + n) * K], K, lmask, nl,
                                           r, slot))
            i += n
        return tuple(torch.cat(x, 0) for x in zip(*out))

    def caption_with_rollout(self, image, layers=(0, 1, 2, 3), residual=0.5, slot=0, want_tag=False, **over):
        """Greedy captions and where each of their words looked on the image's patches: per chunk of images the encoder with its
        attention written out, the prefill, the greedy loop, then rollout_maps' pass on the loop's own output (the token chosen at the
        last position handed over as last_tok).  -> (ids (B, 1, L), logprobs (B, 1), patches (B, L, 24, 24), cls_mass (B, L),
        text_mass (B, L)); the maps are rollout_maps' (see there for what they are).  want_tag: tag_rollout's map of the same encoder
        pass behind them, (B, 24, 24) and its cls_mass (B,)."""
        from . import rollout as R
        r, lmask = R.check_residual(residual), self._layer_mask(layers)
        o = self._rollout_options('caption_with_rollout', slot, over)
        nl, chunks = bin(lmask).count('1'), self._image_chunks(image, R.N_BLOCKS, False)
        if len(chunks) == 1:
            _, _, grid, cls, text, ids, lp, *tag = self._rollout_chunk(image, o, None, None, 1, lmask, nl, r, slot, want_tag)
            return (ids, lp, grid, cls, text) + tuple(tag)
        # more images than one engine call's maps buffer holds: the captions are those of ONE generate() over the whole batch (so
        # that they do not depend on the chunking), then every chunk is encoded again with its attention written out
        ids, lp, last = self.run(image, o, slot=slot, want_last=True)
        out, i = [], 0
        for img in chunks:
            n = img.shape[0]
            out.append(self._rollout_chunk(img, o, ids[i:i + n, 0], last[i:i + n], 1, lmask, nl, r, slot, want_tag)[2:])
            i += n
        return (ids, lp) + tuple(torch.cat(x, 0) for x in zip(*out))

    def generate_cbs(self, image, fsm, num_constraints, num_beams=1, min_constraints_to_satisfy=2, slot=0, **over):
        """Constrained beam search: ViTCAP.generate(use_cbs=True, fsm=fsm, num_constraints=..., min_constraints_to_satisfy=...)
        (modeling_bert.py:1035-1057 -> utils_cbs.py:26-443) -> (ids (B, 1, T), logprobs (B, 1)).  Like the reference's output the
        ids carry NO BOS column and T <= max_length - 1 is the number of words decoded before every one of the batch's
        B * S * num_beams sequences had ended (one host synchronisation reads it).  fsm / num_constraints: vitcap_amd.cbs.batch_fsm."""
        if fsm is None or num_constraints is None:
            self.gen_options(use_cbs=True, fsm=fsm, num_constraints=num_constraints)       # raises, naming what is missing
        if fsm.shape[0] != image.shape[0] or num_constraints.shape[0] != image.shape[0]:
            raise AssertionError('fsm / num_constraints are for %d images, the batch has %d (modeling_bert.py:953)'
                                 % (fsm.shape[0], image.shape[0]))
        o = self.gen_options(use_cbs=True, fsm=fsm, num_constraints=num_constraints, num_beams=int(num_beams), num_keep_best=1,
                             min_constraints_to_satisfy=int(min_constraints_to_satisfy), do_sample=False, num_return_sequences=1, **over)
        ids, lp = self.run(image, o, slot=slot)
        n_pred = int(self.tap('cbs_npred', image.shape[0], (1,), dtype=torch.int32, slot=slot, opts=o)[0])
        return ids[:, :, :n_pred].contiguous(), lp

    def generate_async(self, image, num_beams=1, length_penalty=1.0, lane=0, opts=None):
        """Captions through a two-slot software pipeline: the ViT encoder + decoder prefill of THIS batch run on one
        HIP stream while the decode steps of the PREVIOUS batch run on another.  The decode phase is a chain of small
        latency-bound kernels that leaves most of the chip idle; the encoder is MFMA-bound and has a tail at every
        GEMM -- interleaved they fill each other's gaps (tools/pipe_bench.py).  The large GEMMs run one tile per workgroup
        here (vitcap_gen_opts.gemm_mode = TILES, a per-call option).
        Returns a handle; `.result()` waits for this batch only and gives (ids, logprobs).  Results are identical to run()."""
        dev = self._check_image(image)
        if opts is None:
            opts = self.gen_options(gemm_mode=L.GEMM_TILES, num_beams=int(num_beams), length_penalty=float(length_penalty),
                                    num_keep_best=1, do_sample=False, num_return_sequences=1)
        pipes = self.__dict__.setdefault('_pipes', {})
        pipe = pipes.get(lane)
        if pipe is None:
            import os
            prio = int(os.environ.get('VITCAP_DECODE_PRIORITY', '-1'))     # -1 = high: the latency-bound chain goes first
            pipe = pipes[lane] = {'enc': role_stream(dev, 'enc%d' % lane, lambda: _encode_stream(dev)),
                                  'dec': role_stream(dev, 'dec%d' % lane, lambda: torch.cuda.Stream(dev, priority=prio)),
                                  'done': [None, None], 'n': 0}
        slot = pipe['n'] % 2
        pipe['n'] += 1
        B = image.shape[0]
        ws, need = self._workspace(B, dev, slot='pipe%d_%d' % (lane, slot), opts=opts, wait=pipe['done'][slot])
        cur = torch.cuda.current_stream(dev)
        ready = torch.cuda.Event()
        ready.record(cur)
        image.record_stream(pipe['enc'])
        with torch.cuda.stream(pipe['enc']):
            pipe['enc'].wait_event(ready)
            if pipe['done'][slot] is not None:
                pipe['enc'].wait_event(pipe['done'][slot])         # the slot's previous decode has drained
            self._encode_prefill(image, opts, ws, need, _stream(pipe['enc']))
            filled = torch.cuda.Event()
            filled.record(pipe['enc'])
        with torch.cuda.stream(pipe['dec']):
            pipe['dec'].wait_event(filled)
            ids, lp = self._out_buffers(B, opts, dev)
            self._decode('', None, B, opts, ws, need, ids, lp, (None,), stream=_stream(pipe['dec']))
            # blocking: a host thread that waits for this batch SLEEPS (hipEventBlockingSync) instead of spinning on a core -- under a
            # CPU quota (the GPU pool gives 16 cores) spinning waiters starve the JPEG decode workers of the loader
            done = torch.cuda.Event(blocking=True)
            done.record(pipe['dec'])
        pipe['done'][slot] = done
        return _Pending(ids, lp, done, image)

    def prime_pipeline(self, B, device, num_beams=1, lane=0, opts=None):
        """Allocate (and touch) both workspaces of generate_async's two-slot pipeline for batches of B images, so that no
        allocation lands inside a caller's timed or latency-critical region.  No kernels of the captioning path run."""
        if self._packed is None:
            self.pack(device)
        if opts is None:
            opts = self.gen_options(gemm_mode=L.GEMM_TILES, num_beams=int(num_beams), num_keep_best=1, do_sample=False,
                                    num_return_sequences=1)
        for slot in range(2):
            ws, _ = self._workspace(B, self._packed[2], slot='pipe%d_%d' % (lane, slot), opts=opts)
            ws.zero_()

    def tap(self, name, B, shape, dtype=torch.float32, slot=0, opts=None):
        """Copy of an engine workspace buffer after the last run() on `slot` (parity taps)."""
        if opts is None:
            last = getattr(self, '_last', None)
            opts = last[1] if last is not None and last[0] == slot and last[2] == B else self.gen_options()
        ws, _ = self._workspace(B, self._packed[2], slot, opts)
        p = lib.vitcap_engine_tap(self._engine, name.encode(), _p(ws), B, C.byref(opts))
        if not p:
            raise KeyError(name)
        off = p - ws.data_ptr()
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        return ws[off:off + n].view(dtype).view(shape).clone()

    def graph_count(self):
        return int(lib.vitcap_engine_graph_count(self._engine)) if self._engine is not None else 0

    def forward(self, data):
        """Test-time contract of the reference wrapper (..._bertemb.py:87-184)."""
        data = dict(data.items())
        data.pop('key', None)
        if self.training:
            # a16 train branch (..._bertemb.py:93-171): returns {'masked_loss': loss}.  Forward and backward are one fused
            # pass of the HIP training engine; loss.backward() (what do_train_dict calls, trainer.py:119) finalises the
            # gradients already sitting in the engine's flat buffer, engine.optimizer_step() is clip + AdamW + schedule.
            eng = getattr(self, 'train_engine', None)
            if eng is None:
                raise RuntimeError('training-mode forward needs a vitcap_amd.train.TrainEngine(model, ...) attached')
            return eng.loss_dict(data)
        te = self.test_extra_input
        over = {}
        # a caption prefix per image: batch key `prefix_ids` (B, P), or the same for every call in test_extra_input
        prefix = data.pop('prefix_ids', te.get('prefix_ids'))
        if prefix is not None:
            self.refuse_forced_search(te.get('num_beams', 1), te.get('use_cbs', False))
        if te.get('do_sample', False):
            # every forward() call advances the stream of draws, like consecutive torch.multinomial calls would
            self._sample_calls = getattr(self, '_sample_calls', 0) + 1
            over['seed'] = int(te.get('seed', 0)) + 0x632be5ab * (self._sample_calls - 1)
        nret = int(te.get('num_return_sequences', 1) or 1)
        image = data['image']
        if nret > 8 and te.get('do_sample', False) and int(te.get('num_beams', 1) or 1) == 1:
            # beyond the engine's sequences-per-image limit: expand the inputs like the reference does (modeling_bert.py:976-994)
            image = image.repeat_interleave(nret, 0).contiguous()
            over['num_return_sequences'] = 1
            if prefix is not None and torch.as_tensor(prefix).shape[0] * nret == image.shape[0]:
                prefix = torch.as_tensor(prefix).repeat_interleave(nret, 0)
        if te.get('use_cbs', False):
            # the batch carries the machines (modeling_bert.py:932: generate's own kwargs)
            n_tag = self.check_text_inputs(data, int(te.get('max_length', L.MAXLEN)))
            if n_tag:
                raise NotImplementedError('use_cbs with tag tokens visible to the caption is not built')
            return self.generate_cbs(image, data.get('fsm', te.get('fsm')), data.get('num_constraints', te.get('num_constraints')),
                                     num_beams=int(te.get('num_beams', 1) or 1),
                                     min_constraints_to_satisfy=int(data.get('min_constraints_to_satisfy',
                                                                             te.get('min_constraints_to_satisfy', 2))))
        opts = self.gen_options(**over)
        n_tag = self.check_text_inputs(data, opts.max_length)
        if n_tag != opts.tag_visible:
            if opts.tag_visible:
                raise ValueError('test_extra_input tag_visible=%d but the attention_mask shows %d tag slots' % (opts.tag_visible, n_tag))
            opts = self.gen_options(tag_visible=n_tag, **over)      # the caller's mask decides
        forced, sf = self._prefix_forced(prefix, image.shape[0], opts.seqs_per_image, opts.max_length)
        return self.run(image, opts, forced=forced, score_forced=sf)
