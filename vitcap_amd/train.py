"""Cross-entropy training step of ViTCAP on MI355X.

Mirrors ``do_train_dict`` (src/tools/opt/trainer.py:95-142) around ``ImageCaptioning.forward`` in training mode
(..._bertemb.py:87-171 -> ViTCAP.encode_forward(is_training=True), modeling_bert.py:751-807): forward, masked-token
label-smoothed loss, backward, global-norm clip over ALL parameters, the reference's AdamW (decay after the update)
on its ten parameter groups, linear LR decay.  Every FLOP runs in the hand-written HIP kernels; this module only
sequences launches and owns the buffers (torch is used for allocation, views, row gathers/copies and the RCCL
all-reduce).

What is computed (identical loss and gradients to the reference, less dead work):
* the decoder runs on [578 visual | 20 caption] rows per image.  The reference's 50 tag slots and the padding rows
  are attended by nothing that reaches the loss (seq2seq mask with text_b='', dataset.py:377-390), so their rows are
  not materialised; caption row r attends all visual rows and caption rows <= r.
* attention dropout of the decoder (attention_probs_dropout_prob = 0.1, active in the reference's training mode,
  modeling_bert.py:330-333) is applied inside the attention kernels with a counter-based keep decision
  (csrc/rng.h) that the forward and both backward passes recompute -- no mask is stored.  `attn_dropout=0` gives the
  deterministic step the goldens of tests/golden/make_golden_train.py are defined on.
* the tag head runs forward only: `tag_loss` is reported, never back-propagated by this pipeline
  (..._bertemb.py:170-171), and bert.pooler / bert.tag_logit / bert.extra_embeddings / caption_pooler / image head
  receive no gradient.

Gradients of a data-parallel job are summed with ONE RCCL all-reduce per bucket over the flat fp32 gradient buffer
(layout = reverse execution order friendly), launched on a side stream as soon as a bucket's last producer ran.
"""
import ctypes as C
import math
import os

import torch

from . import _lib as L
from . import ops
from . import weights as W
from ._lib import check, lib

CH = 1024           # optimizer chunk (elements)
NV = 577
SV = 578
T = 20
LR = SV + T         # decoder rows per image (masked-token step)
QLO = (SV // 128) * 128     # first 128-row query block of the decoder that holds text rows


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lowbias32(x):
    x &= 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def mix32(h, v):
    """vc_mix of csrc/rng.h on Python ints."""
    return _lowbias32(h ^ ((v + 0x9e3779b9 + (h << 6) + (h >> 2)) & 0xffffffff))


def param_groups(names, base_lr, weight_decay, lr_multiplier):
    """name -> (lr, wd) or None (not owned by the optimizer); ..._bertemb.py:280-356."""
    out = {}
    for n in names:
        if n.startswith('module.cls.'):
            out[n] = None
            continue
        low = n.startswith('module.bert.encoder.tag_blocks.') or n.startswith('module.bert.pooler.') \
            or n.startswith('module.bert.tag_logit.')
        if n.startswith('module.bert.encoder.blocks.'):
            low = int(n.split('.')[4]) < 8
        wd = 0.0 if ('bias' in n or 'LayerNorm.weight' in n) else weight_decay
        out[n] = (base_lr * (lr_multiplier if low else 1.0), wd)
    return out


def flat_layout(tied):
    """Flat fp32 parameter / gradient layout: (order, offset, shape, total).  Every unique tensor is padded to CH
    elements (optimizer chunks carry lr / weight decay); the decoder's q|k|v weights, then their biases, are contiguous
    so one GEMM / one bias vector covers the three projections."""
    spec = W.state_dict_spec()
    off, shape, order = {}, {}, []
    for k in spec:
        if tied and k == W.TIED_DST:
            continue
        if '.attention.self.' in k:
            if k.endswith('query.weight'):          # q|k|v weights, then q|k|v biases, contiguous
                pre = k[:-len('query.weight')]
                order += [pre + n + '.weight' for n in ('query', 'key', 'value')]
                order += [pre + n + '.bias' for n in ('query', 'key', 'value')]
            continue
        order.append(k)
    cur = 0
    for k in order:
        shp = spec[k][0]
        n = int(torch.Size(shp).numel())
        off[k], shape[k] = cur, shp
        is_qk_bias = k.endswith('attention.self.query.bias') or k.endswith('attention.self.key.bias')
        cur = cur + n if is_qk_bias else (cur + n + CH - 1) // CH * CH      # q|k|v biases stay contiguous (2304 -> 3 chunks)
    nflat = (cur + CH - 1) // CH * CH
    if tied:
        off[W.TIED_DST], shape[W.TIED_DST] = off[W.TIED_SRC], shape[W.TIED_SRC]
    return order, off, shape, nflat


def chunk_hparams(order, off, shape, nflat, pg):
    """Per-chunk (lr, weight decay) of the fused AdamW; lr 0 = the tensor is not stepped (no gradient in the reference, or
    not owned by its optimizer).  A chunk never mixes tensors with different hyper-parameters."""
    lr = torch.zeros(nflat // CH)
    wd = torch.zeros(nflat // CH)
    owner = {}
    for k in order:
        n = int(torch.Size(shape[k]).numel())
        c0, c1 = off[k] // CH, (off[k] + n + CH - 1) // CH
        hp = (0.0, 0.0) if (pg[k] is None or k.startswith(NO_GRAD_PREFIXES)) else (float(pg[k][0]), float(pg[k][1]))
        for c in (c0, c1 - 1):
            if owner.setdefault(c, hp) != hp:
                raise AssertionError('optimizer chunk %d shared by tensors with different lr / weight decay (%s)' % (c, k))
        lr[c0:c1], wd[c0:c1] = hp
    return lr, wd


NO_GRAD_PREFIXES = ('module.bert.extra_embeddings.', 'module.bert.tag_logit.', 'module.bert.pooler.',
                    'module.bert.caption_pooler.', 'image_encoder.module.head.')


def grad_stage(key):
    """Backward stage after which the gradient of `key` is final, or None if it never receives one.  Stages complete in
    the order of GRAD_STAGES; two consecutive layers share a stage so a bucket is ~57 MB (ring all-reduce over xGMI is
    per-link bound: few large messages)."""
    if key.startswith(NO_GRAD_PREFIXES):
        return None
    if key.startswith('module.cls.'):
        return 'cls'
    if key.startswith('module.bert.decoder.layer.'):
        return 'dec%d' % (int(key.split('.')[4]) // 2)
    if key.startswith('module.bert.embeddings.'):
        return 'emb'
    if key.startswith('module.bert.encoder.tag_blocks.'):
        return 'tag%d' % (int(key.split('.')[4]) // 2)
    if key.startswith('module.bert.encoder.blocks.'):
        return 'blk%d' % (int(key.split('.')[4]) // 2)
    if key.startswith('image_encoder.module.'):
        return 'patch'
    raise KeyError(key)


GRAD_STAGES = ['cls', 'dec1', 'dec0', 'emb', 'tag1', 'tag0', 'blk5', 'blk4', 'blk3', 'blk2', 'blk1', 'blk0', 'patch']


def grad_buckets(order, off, shape):
    """stage -> list of (start, end) element ranges of the flat gradient (adjacent tensors of a stage merged)."""
    out = {st: [] for st in GRAD_STAGES}
    for k in order:
        st = grad_stage(k)
        if st is None:
            continue
        n = int(torch.Size(shape[k]).numel())
        a, b = off[k], off[k] + n
        runs = out[st]
        if runs and a - runs[-1][1] < CH:       # only chunk padding in between
            runs[-1] = (runs[-1][0], b)
        else:
            runs.append((a, b))
    return out


def train_text_inputs_ok(batch):
    """0-d bool tensor (on the device the batch's attention_mask lives on): True when `attention_mask` (B, L, L) and
    `masked_pos` describe the training mask the kernels implement -- tril on the real caption rows ([CLS] .. [SEP]) of the
    first 20 slots and zeros elsewhere, masked positions on real rows only (TrainEngine.check_text_inputs).  None when the
    batch carries no attention_mask (or is a self-critical batch, which has no text inputs)."""
    am = batch.get('attention_mask')
    if am is None or 'sample_ids' in batch:
        return None
    if am.dim() != 3 or am.shape[1] != am.shape[2] or am.shape[1] < T:
        raise NotImplementedError('training attention_mask must be the (B, L, L) seq2seq mask with L >= %d, got %s '
                                  '(mask_type bidirectional is not built)' % (T, tuple(am.shape)))
    Lm = am.shape[1]
    a = am != 0
    n_real = a[:, :T, :T].diagonal(dim1=1, dim2=2).sum(1)                         # real caption rows: [CLS] .. [SEP]
    idx = torch.arange(Lm, device=am.device)
    real = idx.view(1, Lm) < n_real.view(-1, 1)                                   # (B, L)
    want = (idx.view(1, 1, Lm) <= idx.view(1, Lm, 1)) & real.unsqueeze(2) & real.unsqueeze(1)
    ok = (a == want).all()
    mp = batch.get('masked_pos')
    if mp is not None:
        ok = ok & ((mp != 0).to(am.device) <= real[:, :mp.shape[1]]).all()
    return ok


class _FusedLoss(torch.autograd.Function):
    """Loss tensor of a fused forward+backward: .backward() scales the gradients the engine already holds."""
    @staticmethod
    def forward(ctx, anchor, engine, batch):
        ctx.engine = engine
        loss, _ = engine.forward_backward(batch)
        engine._pending = True
        return loss.detach().clone()

    @staticmethod
    def backward(ctx, g):
        eng = ctx.engine
        if not eng._pending:
            raise RuntimeError('backward() called twice on the loss of one fused training forward')
        eng._pending = False
        # forward_backward() already launched the per-bucket all-reduce (+ 1/world scaling) of this same flat buffer on the
        # communication stream: join it BEFORE touching G on the compute stream, or the multiply races with the reduce and the
        # ranks end up with different gradients
        eng.all_reduce_grads()
        # d(sum of losses)/d(masked_loss): 1 in do_train_dict (trainer.py:117-119).  Applied on the device whatever its value --
        # testing it on the host would be a device-to-host synchronisation per step right behind the gradient exchange
        eng.G.mul_(g.to(eng.G.dtype))
        return None, None, None


class _Rec(object):
    """Plain record of views: one layer's weights, or one weight's w / wt / b / gw / gb (TrainEngine._bind_layers)."""
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Step(object):
    """Per-step context of TrainEngine._fb_gen (the role Enq plays in csrc/engine.cpp): shapes, flags, dropout seeds and
    probabilities, and the activations one phase of the step leaves for a later one (set by the phase that produces them)."""
    def __init__(self, eng, batch, capture):
        self.batch = batch
        self.Be = batch['image'].shape[0]                # images the encoder runs on
        self.KS = int(batch.get('seq_per_image', 1))     # decoder sequences per image (self-critical step: the samples of an image
        self.B = self.Be * self.KS                       # share its encoder pass; their visual-row gradients are summed before its backward)
        self.scst = 'sample_ids' in batch
        self.TP = (T - 1) if self.scst else 0            # probe rows per sequence
        self.TT = T + self.TP                            # text rows per sequence
        self.LR = SV + self.TT                           # decoder rows per sequence
        self.M, self.Md = self.Be * NV, self.B * self.LR
        self.prune = eng.prune_dead_rows
        self.ph, self.pd = eng.hidden_dropout, eng.attn_dropout
        self.seed = mix32(eng.dropout_seed, 0 if capture else eng.step_no)
        self.dseed = [mix32(self.seed, l) for l in range(4)]      # attention dropout: per step, per layer
        self.saved, self.dsaved = {}, []                 # ViT activations by block record; decoder activations by layer

    def hseed(self, l, site):
        """Hidden dropout: per step, per layer (4 = embeddings), per site (1 attention.output, 2 output, 3 embeddings)."""
        return mix32(mix32(self.seed, 16 + l), site)

class TrainEngine(object):
    def __init__(self, model, device='cuda', base_lr=1e-4, weight_decay=0.05, lr_multiplier=0.1, clip=1.0, max_iter=1000,
                 label_smoothing=0.1, dist=None, attn_dropout=0.1, dropout_seed=0, tag_loss='focal', hidden_dropout=0.0):
        """tag_loss: 'focal' (the shipped YAML's `loss: focal`: summed focal loss) or 'bce' (any other `loss`: BCEWithLogitsLoss mean,
        modeling_bert.py:713-717) -- the reported `tag_loss`, never back-propagated by this pipeline."""
        if tag_loss not in ('focal', 'bce'):
            raise ValueError("tag_loss must be 'focal' or 'bce', got %r" % (tag_loss,))
        self.tag_loss = tag_loss
        self.model = model
        self.dev = torch.device(device)
        if self.dev.index is None:
            self.dev = torch.device('cuda', torch.cuda.current_device())
        self.clip, self.max_iter, self.eps_ls = clip, max_iter, label_smoothing
        self.dist = dist
        self.attn_dropout = float(attn_dropout)
        self.hidden_dropout = float(hidden_dropout)     # BertConfig.hidden_dropout_prob (the pipeline's drop_out): embeddings, both dense outputs per layer
        # outputs nobody reads are not computed: rows 1..576 of the last tag block, the visual rows of the last decoder layer
        # (forward and backward; same loss and gradients).  VITCAP_TRAIN_FULL_ROWS=1 computes them anyway (A/B measurements).
        self.prune_dead_rows = os.environ.get('VITCAP_TRAIN_FULL_ROWS', '0') != '1'
        rank = dist.get_rank() if (dist is not None and dist.is_initialized()) else 0
        self.dropout_seed = mix32(int(dropout_seed) & 0xffffffff, rank)      # every rank drops differently
        self.step_no = 0
        self.lr_scale = 1.0
        tied = model.tie_weights
        order, self.off, self.shape, self.nflat = flat_layout(tied)
        self.P = torch.zeros(self.nflat, device=self.dev)
        self.G = torch.zeros(self.nflat, device=self.dev)
        self.M = torch.zeros(self.nflat, device=self.dev)
        self.V = torch.zeros(self.nflat, device=self.dev)
        sd = model.state_dict()
        for k in order:
            self.p(k).copy_(sd[k])
        pg = param_groups(order, base_lr, weight_decay, lr_multiplier)
        lr, wd = chunk_hparams(order, self.off, self.shape, self.nflat, pg)
        self.chunk_lr, self.chunk_wd = lr.to(self.dev), wd.to(self.dev)
        self.gsumsq = torch.zeros(1, device=self.dev)
        self.loss_buf = torch.zeros(2, device=self.dev)      # [masked_loss, tag_loss]
        self._gemm_w = {}
        self._ct_table = None
        # DDP's wrap broadcasts rank 0's parameters and buffers to every replica (uni_pipeline.py:497-505): ranks that loaded different
        # files (or none) must not train as one model.  The Adam moments follow after a resume (sync_from_rank0).
        from .dist_util import BucketedAllReduce, broadcast_from_rank0
        self.synced_bytes = broadcast_from_rank0([self.P], dist)
        # device-side NaN / Inf watch on the loss and the gradient norm (trainer.py:134-137 raises on `losses != losses` every step;
        # here the flag is read at the host synchronisations that exist anyway: every 50 steps, before a snapshot, after the last step)
        self._nan_bad = torch.zeros((), dtype=torch.int32, device=self.dev)
        self._nan_first = torch.full((), -1, dtype=torch.int32, device=self.dev)
        self.nan_dump = None              # callable(name) that saves the context (the pipeline passes its Checkpointer.save); default: torch.save here
        self.nan_dump_dir = '.'
        self.refresh_weights()
        self._bind_layers()
        self.reducer = BucketedAllReduce(self.G, grad_buckets(order, self.off, self.shape), GRAD_STAGES, dist)
        self._anchor = torch.zeros(1, device=self.dev, requires_grad=True)
        self._pending = False
        self.use_graphs = os.environ.get('VITCAP_TRAIN_GRAPH', '0') == '1'      # train_step() replays captured segments (graph mode below)
        self._graphs = {}
        model.__dict__['train_engine'] = self          # ImageCaptioning.forward (training mode) routes here

    def loss_dict(self, batch):
        """What ImageCaptioning.forward returns in training mode (..._bertemb.py:170-171)."""
        return {'masked_loss': _FusedLoss.apply(self._anchor, self, batch)}

    def check_text_inputs(self, batch, host_read=True):
        """The training kernels hard-wire the mask CaptionTensorizer.tensorize_ab builds for a caption without text_b
        (dataset.py:377-390, mask_type seq2seq): token row i attends the visual rows and token rows <= i; rows behind the
        caption's [SEP] are padding whose outputs the loss never reads.  A caller's `attention_mask` (B, L, L) is verified
        against exactly that -- tril on the real caption rows, zeros elsewhere (no text_b columns, no seq2seq_off diagonal,
        no bidirectional vector) -- and `masked_pos` must select real caption rows only; anything else is refused instead of
        being trained with a different mask than the caller asked for.
        Host tensors (what the loader yields) are checked on the host.  Tensors that already live on the device are checked
        with a host read on the first step only; afterwards the comparison runs on their stream into a device counter that is
        read every 50 steps (a per-step read would be a device-to-host synchronisation in front of every step).
        host_read=False (the step is being captured into a graph): the device-side comparison only, read by flush_text_check
        outside the graph."""
        ok = train_text_inputs_ok(batch)
        if ok is None:
            return
        if host_read and (not ok.is_cuda or not getattr(self, '_text_checked', False)):
            self._text_checked = True
            if not bool(ok):
                raise NotImplementedError(
                    'training attention_mask / masked_pos do not describe the mask the HIP training kernels implement (tril on the '
                    'real caption rows of the first %d slots, zeros elsewhere: tensorize_ab without text_b, mask_type seq2seq, '
                    'dataset.py:377-390)' % T)
            return
        self._text_counter(ok.device).add_((~ok).to(torch.int32))
        if host_read and self.step_no % 50 == 49:
            self.flush_text_check()

    def _text_counter(self, device):
        """Device-side count of the batches whose text tensors the kernels do not implement (read by flush_text_check)."""
        if getattr(self, '_text_bad', None) is None:
            self._text_bad = torch.zeros((), dtype=torch.int32, device=device)
        return self._text_bad

    def sync_from_rank0(self):
        """Parameters AND Adam moments of every rank := rank 0's (after a resume: a rank that read a stale or different snapshot would
        otherwise keep its own moments); bf16 operand copies rebuilt.  No-op without a process group."""
        from .dist_util import broadcast_from_rank0
        n = broadcast_from_rank0([self.P, self.M, self.V], self.dist)
        if n:
            self.refresh_weights()
        return n

    def _watch_nan(self):
        """Enqueued once per step behind vitcap_sumsq: counts the steps whose loss or gradient norm is not finite (no host read)."""
        bad = ~(torch.isfinite(self.loss_buf[0]) & torch.isfinite(self.gsumsq[0]))
        self._nan_first.copy_(torch.where(bad & (self._nan_first < 0), torch.full_like(self._nan_first, self.step_no), self._nan_first))
        self._nan_bad += bad.to(torch.int32)

    def flush_nan_check(self):
        """trainer.py:134-137: `if losses != losses: checkpointer.save("NaN_context_{rank}"); raise RuntimeError('NaN encountered!')`.
        The reference tests the loss on the host after every step; here the device-side flag of _watch_nan (loss OR gradient norm not
        finite -- an Inf gradient reaches the parameters one step before the loss shows it) is read where the host waits anyway."""
        if int(self._nan_bad) == 0:
            return
        first, n = int(self._nan_first), int(self._nan_bad)
        self._nan_bad.zero_()
        self._nan_first.fill_(-1)
        rank = self.dist.get_rank() if (self.dist is not None and self.dist.is_initialized()) else 0
        name = 'NaN_context_{}'.format(rank)
        import logging
        logging.info('NaN encountered! (first at step %d, %d step(s) since the last check)', first, n)
        if self.nan_dump is not None:
            self.nan_dump(name)
        else:
            torch.save({'model': self.state_dict(), 'iteration': self.step_no, 'first_bad_step': first,
                        'optimizer': self.optimizer_state_dict(), 'scheduler': self.scheduler_state_dict()},
                       os.path.join(self.nan_dump_dir, name + '.pt'))
        raise RuntimeError('NaN encountered!')

    def flush_text_check(self):
        """Reads the device-side counter of batches whose text tensors the kernels do not implement (one host synchronisation) and
        the NaN watch (flush_nan_check).
        Called every 50 steps, and by the pipeline before every checkpoint it saves and after the last step (otherwise a
        snapshot could be written from up to 49 steps trained on the hard-wired mask, and the final steps were never reported)."""
        self.flush_nan_check()
        bad = getattr(self, '_text_bad', None)
        if bad is not None and int(bad) != 0:
            self._text_bad = None
            raise NotImplementedError('a training batch since the last check carried an attention_mask / masked_pos the HIP '
                                      'training kernels do not implement (TrainEngine.check_text_inputs)')

    # ------------------------------------------------------------------ views
    def p(self, k):
        n = int(torch.Size(self.shape[k]).numel())
        return self.P[self.off[k]:self.off[k] + n].view(self.shape[k])

    def g(self, k):
        n = int(torch.Size(self.shape[k]).numel())
        return self.G[self.off[k]:self.off[k] + n].view(self.shape[k])

    def state_dict(self):
        return {k: self.p(k).detach().clone() for k in W.state_dict_spec()}

    # optimizer / scheduler payloads of the reference checkpoint (src/tools/opt/checkpoint.py:60-75 saves
    # optimizer.state_dict() and scheduler.state_dict() next to the model; trainer.py:95 resumes from 'iteration')
    def optimizer_state_dict(self):
        return {'format': 'vitcap_amd.flat_adamw.v1', 'nflat': self.nflat, 'step': self.step_no,
                'exp_avg': self.M.detach().cpu(), 'exp_avg_sq': self.V.detach().cpu()}

    def load_optimizer_state_dict(self, sd):
        if sd.get('format') != 'vitcap_amd.flat_adamw.v1' or int(sd.get('nflat', -1)) != self.nflat:
            raise ValueError('optimizer state of another layout (%r, %r elements; this engine holds %d)'
                             % (sd.get('format'), sd.get('nflat'), self.nflat))
        self.M.copy_(sd['exp_avg'])
        self.V.copy_(sd['exp_avg_sq'])
        self.step_no = int(sd['step'])

    def scheduler_state_dict(self):
        return {'last_epoch': self.step_no, 'lr_scale': self.lr_scale, 't_total': self.max_iter}

    def load_scheduler_state_dict(self, sd):
        self.lr_scale = float(sd['lr_scale'])

    def load_model_state_dict(self, sd):
        """Parameters from a checkpoint's 'model' dict (resume): flat fp32 master copy + the bf16 GEMM operands."""
        for k in W.state_dict_spec():
            if k in sd:
                self.p(k).copy_(sd[k])
        self.refresh_weights()

    # ------------------------------------------------------------------ bf16 operands of the GEMMs
    def _matrices(self):
        """(name, first key, N, K, pad_N): GEMM weights = the matrix rows of W.weights_table() this engine trains (decoder q|k|v are
        one [2304,768] matrix in the flat layout; a tied caption decoder is the word embedding's pair)."""
        spec, out = W.state_dict_spec(), []
        for f in W.weights_table():
            if f.kind != 'mat' or f.optional or (f.tied_to and self.model.tie_weights):
                continue
            N, K = f.rows_cols(spec)
            out.append((f.name, f.keys[0], N, K, f.pad or (N + 7) // 8 * 8))
        return out

    def refresh_weights(self):
        """fp32 masters -> bf16 W[N][K] and W^T[K][N] (forward / dgrad operands); called after every optimizer step.  ONE launch for
        all matrices (vitcap_cast_transpose_multi over a device-resident table built once): as ~110 launches of a few microseconds
        each they were launch floor (0.74 ms of kernel time per step; same-box A/B 55.78 -> 55.44 ms)."""
        if self._ct_table is None:
            items, tile0 = [], 0
            for name, key, N, K, padN in self._matrices():
                self._gemm_w[name] = (torch.zeros(padN, K, device=self.dev, dtype=torch.bfloat16),
                                      torch.zeros(K, padN, device=self.dev, dtype=torch.bfloat16))
                wb, wt = self._gemm_w[name]
                assert K % 64 == 0 and padN >= N and padN % 8 == 0
                src = self.P[self.off[key]:self.off[key] + N * K]
                items.append(L.CtItem(src.data_ptr(), wb.data_ptr(), wt.data_ptr(), N, K, padN, tile0))
                tile0 += ((N + 63) // 64) * (K // 64)
            raw = bytes((L.CtItem * len(items))(*items))
            self._ct_table = (torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.dev), len(items), tile0)
            if self.model.tie_weights:
                self._gemm_w['cls.dec'] = self._gemm_w['word']
        tab, n, tiles = self._ct_table
        check(lib.vitcap_cast_transpose_multi(_p(tab), n, tiles, _s()), 'cast_transpose_multi')

    def bind_inference(self):
        """Points the model's INFERENCE engine at this engine's own device buffers (bf16 matrices refreshed after every
        optimizer step, fp32 vectors = views of the master buffer): generate() then always decodes with the current
        weights, with no copy -- what the self-critical step needs between its sampling and its gradient pass."""
        def buffer(f):
            if f.optional:
                return None
            if f.kind == 'mat':
                return self.wb(f.name)
            # q|k|v biases are contiguous in the flat layout; the master chunk behind a 30522-vector is zero-padded to 30720 >= VOCAB_PAD
            o = self.off[f.keys[0]]
            return self.P[o:o + (f.pad or sum(int(torch.Size(self.shape[k]).numel()) for k in f.keys))]
        return self.model.bind_weights(buffer, [self], self.dev)

    def wb(self, name):
        return self._gemm_w[name][0]

    def wt(self, name):
        return self._gemm_w[name][1]

    def vec(self, k):
        return self.p(k).view(-1)

    # ------------------------------------------------------------------ parameters of the step, bound once
    def _bind_layers(self):
        """One record per layer with the views the step reads: P, G and the bf16 operand pairs are allocated once and refresh_weights
        rewrites the pairs in place, so the views stay valid for the life of the engine.  Checkpoint keys are spelled here and in
        W.weights_table() only; the step (everything from _fb_gen down) reads blk.fc1.w, blk.fc1.gb, lay.ao_n.g ..."""
        def lin(name, key, rows=None):
            """Dense layer: w = bf16 W[N][K], wt = W^T, b = fp32 bias, gw / gb = their gradients.  rows: N of a matrix that spans
            several checkpoint tensors (decoder q|k|v, contiguous in the flat layout)."""
            w = self.wb(name)
            N, o, ob = rows or self.shape[key + '.weight'][0], self.off[key + '.weight'], self.off[key + '.bias']
            K = w.shape[1]
            return _Rec(w=w, wt=self.wt(name), b=self.P[ob:ob + N], gw=self.G[o:o + N * K].view(N, K), gb=self.G[ob:ob + N])

        def norm(key):
            return _Rec(g=self.vec(key + '.weight'), b=self.vec(key + '.bias'), gg=self.g(key + '.weight').view(-1), gb=self.g(key + '.bias').view(-1))

        def vit(pre):
            return _Rec(n1=norm(pre + '.norm1'), qkv=lin(pre + '.qkv', pre + '.attn.qkv'), proj=lin(pre + '.proj', pre + '.attn.proj'),
                        n2=norm(pre + '.norm2'), fc1=lin(pre + '.fc1', pre + '.mlp.fc1'), fc2=lin(pre + '.fc2', pre + '.mlp.fc2'))

        def bert(pre):
            return _Rec(qkv=lin(pre + '.qkv', pre + '.attention.self.query', rows=2304), ao=lin(pre + '.ao', pre + '.attention.output.dense'),
                        ao_n=norm(pre + '.attention.output.LayerNorm'), i=lin(pre + '.i', pre + '.intermediate.dense'),
                        o=lin(pre + '.o', pre + '.output.dense'), o_n=norm(pre + '.output.LayerNorm'))

        def head(pre, tname, dname, dkey):
            """LM head: t = transform dense, n = its LayerNorm, dec = decoder (bias: the 30522 checkpoint values, unpadded)."""
            dec = _Rec(w=self.wb(dname), wt=self.wt(dname), b=self.vec(pre + '.bias'), gw=self.g(dkey), gb=self.g(pre + '.bias'))
            return _Rec(t=lin(tname, pre + '.transform.dense'), n=norm(pre + '.transform.LayerNorm'), dec=dec)

        self.blocks = [vit('module.bert.encoder.blocks.%d' % i) for i in range(12)]
        self.tag_blocks = [vit('module.bert.encoder.tag_blocks.%d' % i) for i in range(4)]
        self.dec = [bert('module.bert.decoder.layer.%d' % i) for i in range(4)]
        ie, e = 'image_encoder.module.', 'module.bert.embeddings'
        self.patch = lin('patch', ie + 'patch_embed.proj')
        self.pos_embed = _Rec(p=self.p(ie + 'pos_embed').view(NV, 768), g=self.g(ie + 'pos_embed').view(NV, 768))
        self.cls_token = _Rec(p=self.vec(ie + 'cls_token'), g=self.g(ie + 'cls_token').view(-1))
        self.emb = _Rec(word=self.wb('word'), pos=self.wb('pos'), type=self.wb('type'), n=norm(e + '.LayerNorm'),
                        gword=self.g(e + '.word_embeddings.weight'), gpos=self.g(e + '.position_embeddings.weight'),
                        gtype=self.g(e + '.token_type_embeddings.weight'))
        self.pooler = lin('pooler', 'module.bert.pooler.dense')
        self.tag_head = head('module.bert.tag_logit.predictions', 'tag.t', 'tag.dec', 'module.bert.tag_logit.predictions.decoder.weight')
        # the (tied) embedding gradient: the LM head's decoder is its first writer
        self.cls_head = head('module.cls.predictions', 'cls.t', 'cls.dec', W.TIED_SRC if self.model.tie_weights else W.TIED_DST)

    # ------------------------------------------------------------------ helpers
    def _wgrad_tn(self, dy, x, gview, bias_grad):
        """gview[N][K] = dy^T x and bias_grad[N] += column sums of dy, straight from the row-major backward operands
        (LDS transpose reads, no transposed copies); M is split so that about one wave of 256x256 tiles fills the chip.
        bias_grad=None: the kernel that produced dy has already added its column sums (ops.gemm_ex(colsum=),
        ops.layernorm_bwd(dxb_colsum=), ops.cast_bf16_colsum)."""
        N, Kin = gview.shape
        tiles = (N // 256) * (Kin // 256)
        stages = (dy.shape[0] + 63) // 64
        S = max(1, min(stages, 256 // tiles))
        if S == 1:
            ops.gemm_tn(dy, x, 1, slabs=gview.view(1, N, Kin))
        else:
            ops.reduce_slabs(ops.gemm_tn(dy, x, S), gview)
        if bias_grad is not None:
            ops.colsum_bf16(dy, bias_grad)

    def _dgrad_gelu(self, dy, wt, z, bias_grad, fused):
        """dz = (dy @ W) * gelu'(z) (bf16) with the bias gradient of the layer dz is the output gradient of: with `fused`, added by the
        GEMM's own epilogue where the 256x256 kernel runs (M >= 2048); by a separate pass over dz otherwise.  Returns (dz, pending) --
        pending is the bias gradient still to be added by _wgrad_tn, or None."""
        if fused and dy.shape[0] >= 2048:
            return ops.gemm_ex(dy, wt, aux=z, colsum=bias_grad), None
        return ops.gemm_ex(dy, wt, aux=z), bias_grad

    def _ln_bwd(self, x, dy, nrm, eps, dres=None, dxb_colsum=None):
        return ops.layernorm_bwd(x, dy, nrm.g, eps, nrm.gg, nrm.gb, dres=dres, dxb_colsum=dxb_colsum)

    # ------------------------------------------------------------------ forward + backward
    def forward_backward(self, batch):
        """One fused forward + backward (see _fb_gen): drives the stage generator and starts a bucket's gradient exchange after each
        backward stage."""
        self.reducer.begin()
        gen = self._fb_gen(batch)
        while True:
            try:
                stage = next(gen)
            except StopIteration as done:
                return done.value
            self.reducer.stage_done(stage)

    def _fb_gen(self, batch, capture=False):
        """Generator: yields the name of every backward stage right after that stage's last kernel was enqueued (the driver starts the
        stage's gradient exchange there, or -- graph mode -- ends a captured segment), returns (masked_loss, tag_loss).
        capture=True: the body is being recorded into hipGraph segments (train_step_graph): no host synchronisation, dropout seeds
        of step 0 (the per-step variation comes from the device-resident salt, vitcap_set_dropout_salt).

        batch: image (B,3,384,384) fp32/bf16 cuda; input_ids (B,70) int64; masked_pos (B,70) int; masked_ids (B,3) int64;
        label (B,30522) fp32 -- the dict the reference's collate feeds ImageCaptioning.forward in training.
        Accumulates gradients into self.G (zeroed here) and returns (masked_loss, tag_loss) device scalars.

        Self-critical mode (`sample_ids` (B,20) int64 + `sample_weight` (B,) fp32 in the batch instead of the masked-token
        fields): the loss is sum_b sample_weight[b] * mean_t(-log p(sample_ids[b,t] | sample_ids[b,:t], image)) over the
        generated positions, i.e. ScstRewardCriterion with sample_weight = (reward - baseline) / B.  The 19 per-step
        forwards the reference differentiates through (one full re-encode per generated token) collapse into ONE pass:
        the decoder runs on [578 visual | 20 token rows | 19 [MASK] probe rows], probe j sees tokens 0..j."""
        self.check_text_inputs(batch, host_read=not capture)
        st = _Step(self, batch, capture)
        self.G.zero_()
        self.loss_buf.zero_()
        self._patch_fwd(st)
        self._encoder_fwd(st)
        self._tag_head_fwd(st)
        self._decoder_fwd(st)
        if st.scst:
            self._loss_rows_scst(st)
        else:
            self._loss_rows_masked(st)
        self._lm_head(st)
        yield 'cls'
        yield from self._decoder_bwd(st)
        self._embedding_bwd(st)
        yield 'emb'
        yield from self._encoder_bwd(st)
        self._patch_bwd(st)
        yield 'patch'
        return self.loss_buf[0], self.loss_buf[1]

    # ---- ViT block.  cls_only: only row 0 (CLS) of the block's output is ever read -- the last tag block: tag_hidden feeds the pooler
    # and the joint sequence through tag_hidden[:, 0] alone (modeling_bert.py:1424, 1493).  LN1 and the qkv projection run on every
    # row (the CLS query attends all keys, and K/V carry gradient to every row); attention, proj, LN2 and the MLP run for the Be CLS
    # rows, and the block returns / takes (Be,768).
    def _vit_fwd(self, st, blk, xin, cls_only=False):
        h1, _ = ops.layernorm(xin, blk.n1.g, blk.n1.b, 1e-6)
        qkv = ops.gemm_bias_act(h1, blk.qkv.w, blk.qkv.b)
        ao, lse = ops.attn_dense_train(qkv, st.Be, NV, q_range=(0, 1) if cls_only else None)
        if cls_only:
            ao_r = ao.view(st.Be, NV, 768)[:, 0].contiguous()
            xin_r = xin.view(st.Be, NV, 768)[:, 0].contiguous()
        else:
            ao_r, xin_r = ao, xin
        R = ao_r.shape[0]
        xmid = torch.empty(R, 768, device=self.dev)
        ops.gemm_bias_act(ao_r, blk.proj.w, blk.proj.b, residual=xin_r, out=xmid)
        h2, _ = ops.layernorm(xmid, blk.n2.g, blk.n2.b, 1e-6)
        z = torch.empty(R, 3072, device=self.dev, dtype=torch.bfloat16)
        g = ops.gemm_ex(h2, blk.fc1.w, bias=blk.fc1.b, act=L.ACT_GELU_ERF, zout=z)
        xout = torch.empty(R, 768, device=self.dev)
        ops.gemm_bias_act(g, blk.fc2.w, blk.fc2.b, residual=xmid, out=xout)
        st.saved[blk] = (xin, h1, qkv, ao, lse, xmid, h2, z, g, ao_r)
        return xout

    def _vit_bwd(self, st, blk, dxo, cls_only=False):
        """dxo = gradient of the block's output (cls_only: of its CLS rows); returns the gradient of the block's input on all rows (the
        CLS query's attention spreads it over every row through K and V).
        The bias gradients of fc2 / fc1 / proj are column sums of a backward operand.  On all rows each is added by the kernel that
        WRITES that operand (cast, GEMM epilogue at M >= 2048, LayerNorm backward); on the CLS rows by _wgrad_tn's own pass."""
        Be, M = st.Be, st.M
        xin, h1, qkv, ao, lse, xmid, h2, z, g, ao_r = st.saved.pop(blk)
        fused = not cls_only

        def pending(gb):        # the bias gradient _wgrad_tn still has to add
            return None if fused else gb
        dxb = ops.cast_bf16_colsum(dxo, blk.fc2.gb) if fused else ops.cast_bf16(dxo)
        self._wgrad_tn(dxb, g, blk.fc2.gw, pending(blk.fc2.gb))
        dz, pend = self._dgrad_gelu(dxb, blk.fc2.wt, z, blk.fc1.gb, fused)
        self._wgrad_tn(dz, h2, blk.fc1.gw, pend)
        dh2 = ops.gemm_ex(dz, blk.fc1.wt)
        dmf, dmb = self._ln_bwd(xmid, dh2, blk.n2, 1e-6, dres=dxo, dxb_colsum=blk.proj.gb if fused else None)
        self._wgrad_tn(dmb, ao_r, blk.proj.gw, pending(blk.proj.gb))
        dao = ops.gemm_ex(dmb, blk.proj.wt)
        if cls_only:
            dao_all = torch.zeros(Be, NV, 768, device=self.dev, dtype=torch.bfloat16)
            dao_all[:, 0] = dao
            dao = dao_all.view(M, 768)
        dqkv = ops.attn_dense_bwd(qkv, ao, dao, lse, Be, NV, q_range=(0, 1) if cls_only else None)
        self._wgrad_tn(dqkv, h1, blk.qkv.gw, blk.qkv.gb)
        dh1 = ops.gemm_ex(dqkv, blk.qkv.wt)
        if cls_only:
            res = torch.zeros(Be, NV, 768, device=self.dev)
            res[:, 0] = dmf
            dmf = res.view(M, 768)
        dif, _ = self._ln_bwd(xin, dh1, blk.n1, 1e-6, dres=dmf)
        return dif

    # ---- decoder layer.  text_only: only the text rows' outputs are read -- the last layer (LM head on the masked / probe rows); the
    # visual rows' K/V are still needed (and carry gradient), their attention / output / MLP are not: the attention runs for the query
    # blocks from QLO on, everything behind it on the (B*TT) text rows, and the layer returns / takes the gradient of those rows.
    def _text_rows(self, st, x):
        return x.view(st.B, st.LR, 768)[:, SV:].reshape(st.B * st.TT, 768).contiguous()

    def _all_rows(self, st, x_text, dtype=torch.float32):
        """Text rows back at their place among all decoder rows, zeros on the visual rows."""
        x = torch.zeros(st.B, st.LR, 768, device=self.dev, dtype=dtype)
        x[:, SV:] = x_text.view(st.B, st.TT, 768)
        return x.view(st.Md, 768)

    def _dense_residual(self, st, a, lin, res, rows, seed):
        """BertSelfOutput / BertOutput up to their LayerNorm: dropout(dense(a)) + res.  rows = (rows per sequence, first row): where
        the rows of `a` sit in a sequence, for the dropout's counter."""
        out = torch.empty(a.shape[0], 768, device=self.dev)
        if st.ph > 0:
            ops.gemm_bias_act(a, lin.w, lin.b, out=out)
            ops.hidden_dropout(out, res, rows[0], rows[1], seed, st.ph, out=out)
        else:
            ops.gemm_bias_act(a, lin.w, lin.b, residual=res, out=out)
        return out

    def _dense_residual_bwd(self, st, x, dy, nrm, gb, rows, seed, fused):
        """Backward of LayerNorm(dropout(dense) + res) down to the dense output: (fp32 gradient of the LayerNorm input = what the
        residual branch sees, bf16 gradient of the dense output = the masked one under dropout, bias gradient still to be added by
        _wgrad_tn).  fused: the kernel that writes the bf16 operand adds its column sums to gb (the LayerNorm backward, or the cast
        of the masked gradient); otherwise _wgrad_tn does."""
        if st.ph > 0:
            dxf, _ = self._ln_bwd(x, dy, nrm, 1e-12)
            masked = ops.hidden_dropout(dxf, None, rows[0], rows[1], seed, st.ph)
            dxb = ops.cast_bf16_colsum(masked, gb) if fused else ops.cast_bf16(masked)
        else:
            dxf, dxb = self._ln_bwd(x, dy, nrm, 1e-12, dxb_colsum=gb if fused else None)
        return dxf, dxb, (None if fused else gb)

    def _dec_attn_args(self, st, l, text_only):
        return dict(p_drop=st.pd, drop_seed=st.dseed[l], causal_from=SV, mask_from=SV + T if st.scst else 0,
                    q_range=(QLO, st.LR) if text_only else None)

    def _dec_fwd(self, st, l, xd, text_only=False):
        lay = self.dec[l]
        xb = ops.cast_bf16(xd)
        qkv = ops.gemm_bias_act(xb, lay.qkv.w, lay.qkv.b)
        # visual rows attend visual rows; caption row q attends all visual rows and caption rows <= q (one kernel)
        ctx, lse = ops.attn_dense_train(qkv, st.B, st.LR, **self._dec_attn_args(st, l, text_only))
        if text_only:
            ctx_r, xd_r, rows = self._text_rows(st, ctx), self._text_rows(st, xd), (st.TT, SV)
        else:
            ctx_r, xd_r, rows = ctx, xd, (st.LR, 0)
        t1 = self._dense_residual(st, ctx_r, lay.ao, xd_r, rows, st.hseed(l, 1))
        ab, af = ops.layernorm(t1, lay.ao_n.g, lay.ao_n.b, 1e-12, want_f32=True)
        z = torch.empty(t1.shape[0], 3072, device=self.dev, dtype=torch.bfloat16)
        it = ops.gemm_ex(ab, lay.i.w, bias=lay.i.b, act=L.ACT_GELU_ERF, zout=z)
        t2 = self._dense_residual(st, it, lay.o, af, rows, st.hseed(l, 2))
        _, yf = ops.layernorm(t2, lay.o_n.g, lay.o_n.b, 1e-12, want_bf16=False, want_f32=True)
        st.dsaved.append((xb, qkv, ctx, lse, t1, ab, af, z, it, t2, ctx_r))
        return yf

    def _dec_bwd(self, st, l, dy, text_only=False):
        """dy = gradient of the layer's output (text_only: of its text rows); returns the gradient of its input on all rows.  Bias
        gradients as in _vit_bwd: added by the producing kernel on all rows, by _wgrad_tn on the text rows."""
        lay = self.dec[l]
        xb, qkv, ctx, lse, t1, ab, af, z, it, t2, ctx_r = st.dsaved[l]
        fused = not text_only
        rows = (st.TT, SV) if text_only else (st.LR, 0)
        dt2f, dt2b, pend = self._dense_residual_bwd(st, t2, dy, lay.o_n, lay.o.gb, rows, st.hseed(l, 2), fused)
        self._wgrad_tn(dt2b, it, lay.o.gw, pend)
        dz, pend = self._dgrad_gelu(dt2b, lay.o.wt, z, lay.i.gb, fused)       # [rows,3072] bf16
        self._wgrad_tn(dz, ab, lay.i.gw, pend)
        da = ops.gemm_ex(dz, lay.i.wt, residual=dt2f, out_dtype=torch.float32)
        dt1f, dt1b, pend = self._dense_residual_bwd(st, t1, da, lay.ao_n, lay.ao.gb, rows, st.hseed(l, 1), fused)
        self._wgrad_tn(dt1b, ctx_r, lay.ao.gw, pend)
        dctx = ops.gemm_ex(dt1b, lay.ao.wt)
        if text_only:
            dctx = self._all_rows(st, dctx, torch.bfloat16)
        dqkv = ops.attn_dense_bwd(qkv, ctx, dctx, lse, st.B, st.LR, **self._dec_attn_args(st, l, text_only))
        self._wgrad_tn(dqkv, xb, lay.qkv.gw, lay.qkv.gb)
        res = self._all_rows(st, dt1f) if text_only else dt1f     # the residual path reaches the layer input on the rows that ran
        return ops.gemm_ex(dqkv, lay.qkv.wt, residual=res, out_dtype=torch.float32)

    # ---- phases of the step, in order
    def _patch_fwd(self, st):
        st.patches = ops.patch_gather(st.batch['image'])
        st.x = torch.empty(st.M, 768, device=self.dev)
        pos = self.pos_embed.p
        ops.gemm_bias_act(st.patches, self.patch.w, self.patch.b, residual=pos[1:], out=st.x,
                          row_group=576, out_group_rows=NV, out_row_off=1, res_periodic=1)
        check(lib.vitcap_cls_rows(_p(self.cls_token.p), _p(pos), _p(st.x), st.Be, NV, _s()), 'cls_rows')

    def _encoder_fwd(self, st):
        """12 blocks + 4 tag blocks (forking behind block 7), activations kept.  st.x: hidden states; st.xt_cls: CLS rows of the tag branch."""
        x, xt = st.x, None
        for i in range(12):
            if i == 8:
                xt = x
            x = self._vit_fwd(st, self.blocks[i], x)
        for i in range(3):
            xt = self._vit_fwd(st, self.tag_blocks[i], xt)
        if st.prune:
            st.xt_cls = self._vit_fwd(st, self.tag_blocks[3], xt, cls_only=True)
        else:
            st.xt_cls = self._vit_fwd(st, self.tag_blocks[3], xt).view(st.Be, NV, 768)[:, 0].contiguous()
        st.x = x

    def _tag_head_fwd(self, st):
        """Value of tag_loss only (reported, never back-propagated; the self-critical step has no labels)."""
        dev, hd, batch = self.dev, self.tag_head, st.batch
        pin = ops.cast_bf16(st.xt_cls)
        pooled = ops.gemm_bias_act(pin, self.pooler.w, self.pooler.b, act=L.ACT_TANH)
        tgf = ops.gemm_bias_act(pooled, hd.t.w, hd.t.b, act=L.ACT_GELU_ERF, out_dtype=torch.float32)
        tgb, _ = ops.layernorm(tgf, hd.n.g, hd.n.b, 1e-12)
        tbias = torch.zeros(L.VOCAB_PAD, device=dev)
        tbias[:L.VOCAB] = hd.dec.b
        tag_logits = ops.gemm_bias_act(tgb, hd.dec.w, tbias, out_dtype=torch.float32)
        if 'label' in batch:
            label = batch['label'].to(dev).contiguous()
            if self.tag_loss == 'focal':       # FocalLossWithLogitsNegLoss(alpha .5, gamma 1).sum(), modeling_bert.py:713-715, 789-791
                check(lib.vitcap_focal_loss_sum(_p(tag_logits), L.VOCAB_PAD, L.VOCAB, _p(label), 0.5, _p(self.loss_buf[1:]), st.Be, _s()),
                      'focal')
            else:                              # torch.nn.BCEWithLogitsLoss(), modeling_bert.py:716-717
                check(lib.vitcap_bce_logits_mean(_p(tag_logits), L.VOCAB_PAD, L.VOCAB, _p(label), _p(self.loss_buf[1:]), st.Be, _s()), 'bce')

    def _decoder_fwd(self, st):
        """Text embeddings, then the 4 layers on [578 visual | TT text] rows per sequence.  st.text_out: the last layer's text rows."""
        dev, emb, batch = self.dev, self.emb, st.batch
        B, TT, TP, KS, Be = st.B, st.TT, st.TP, st.KS, st.Be
        if st.scst:
            st.sid = batch['sample_ids'].to(dev).view(B, T)
            st.ids20 = torch.cat([st.sid, torch.full((B, TP), 103, dtype=torch.int64, device=dev)], 1).contiguous()   # tokens | [MASK] x19
        else:
            st.ids20 = batch['input_ids'][:, :T].to(dev).contiguous()
        st.pre_emb = torch.empty(B * TT, 768, device=dev)
        xtext = torch.empty(B * TT, 768, device=dev)
        check(lib.vitcap_embed_rows(_p(st.ids20), TT, _p(emb.word), _p(emb.pos), _p(emb.type), _p(emb.n.g), _p(emb.n.b), 1e-12,
                                    _p(st.pre_emb), _p(xtext), None, B * TT, T if st.scst else 0, _s()), 'embed_rows')
        if st.ph > 0:                  # BertEmbeddings: dropout(LayerNorm(...)) on the text rows (device rows SV .. SV + TT - 1 of a sequence)
            ops.hidden_dropout(xtext, None, TT, SV, st.hseed(4, 3), st.ph, out=xtext)
        dx = torch.empty(B, st.LR, 768, device=dev)
        dx[:, 0] = st.xt_cls if KS == 1 else st.xt_cls.repeat_interleave(KS, 0)
        dx[:, 1:SV] = st.x.view(Be, NV, 768) if KS == 1 else st.x.view(Be, NV, 768).repeat_interleave(KS, 0)
        dx[:, SV:] = xtext.view(B, TT, 768)
        xd = dx.view(st.Md, 768)
        for l in range(3):
            xd = self._dec_fwd(st, l, xd)
        if st.prune:
            st.text_out = self._dec_fwd(st, 3, xd, text_only=True)
        else:
            st.text_out = self._dec_fwd(st, 3, xd).view(B, st.LR, 768)[:, SV:].reshape(B * TT, 768)

    def _loss_rows_scst(self, st):
        """Rows of the text grid the loss reads (st.sel), their targets and weights: probe j (grid column T + j) predicts position j+1;
        a position counts while the sequence is unfinished, i.e. up to and including its first [SEP] (modeling_utils.py:853-877);
        coefficient = weight_b / (#counted positions)."""
        dev, B, TT, TP, sid = self.dev, st.B, st.TT, st.TP, st.sid
        tok = sid[:, 1:]
        ended = ((sid[:, :-1] == 102).cumsum(1) > 0)                     # a [SEP] strictly before this position
        unf = ~ended
        mp = torch.zeros(B, TT, dtype=torch.bool, device=dev)
        mp[:, T:] = unf
        cnt = unf.sum(1).clamp(min=1).to(torch.float32)
        wrow = (st.batch['sample_weight'].to(dev).to(torch.float32) / cnt)[:, None].expand(B, TP)
        st.row_w = wrow[unf].contiguous()
        st.tgt = tok[unf].contiguous()
        st.sel = mp.view(-1).nonzero().view(-1)                              # rows of the (B*TT) text grid
        st.n = int(st.sel.numel())
        assert int(st.tgt.numel()) == st.n, 'sample_ids / unfinished mask disagree'
        st.sel_bwd = st.sel

    def _loss_rows_masked(self, st):
        """The same for the masked-token loss, in a static form (no host synchronisation, same shapes every step: graph-capturable).
        Slot (b, j) = the j-th masked position of sample b; masked_ids[b, j] == 0 marks an unused slot (a caption with fewer than 3
        masked tokens).  The used slots are moved to the front in their original order (stable sort), so with every slot used -- the
        synthetic batches -- rows, targets and weights are exactly what `nonzero()` / boolean indexing produced; an unused slot becomes
        a row with weight 0 (zero loss, zero gradient rows: exact zeros in every sum) whose gradient lands in a dummy row behind the
        text grid."""
        dev, B, TT, batch = self.dev, st.B, st.TT, st.batch
        mpos = batch['masked_pos'][:, :T].to(dev) != 0                       # (B, T)
        mids = batch['masked_ids'].to(dev)                                   # (B, J)
        J = mids.shape[1]
        cum = mpos.to(torch.int32).cumsum(1)                                 # 1-based rank of every masked position
        want = torch.arange(1, J + 1, device=dev, dtype=torch.int32).view(1, J, 1)
        tpos = ((cum.unsqueeze(1) == want) & mpos.unsqueeze(1)).to(torch.int32).argmax(2)      # (B, J): position of the j-th masked token
        rows_all = (torch.arange(B, device=dev).view(B, 1) * TT + tpos).view(-1)
        used = (mids != 0).view(-1)
        # a batch whose masked_pos and masked_ids disagree is reported like a bad mask (device counter, TrainEngine.flush_text_check)
        # (counts equal AND the used slots are the leading ones: dataset.py:321-324 pads masked_ids behind the real ids; a zero in
        # front of a real id would pair targets with the wrong rows -- ADVICE r5)
        nm = mpos.sum(1, keepdim=True)
        bad = (nm.view(-1) != (mids != 0).sum(1)).any() | ((mids != 0) != (torch.arange(J, device=dev).view(1, J) < nm)).any()
        self._text_counter(dev).add_(bad.to(torch.int32))
        order = torch.argsort((~used).to(torch.int8), stable=True)
        used_s = used[order]
        st.sel = rows_all[order].contiguous()                                # forward: any valid row index (weight 0 where unused)
        st.sel_bwd = torch.where(used_s, st.sel, torch.full_like(st.sel, B * TT))     # backward: unused slots -> the dummy row
        st.tgt = mids.view(-1)[order].contiguous()
        st.n = B * J
        st.row_w = (used_s.to(torch.float32) / used.sum().clamp(min=1).to(torch.float32)).contiguous()     # 1 / #masked tokens: the mean

    def _lm_head(self, st):
        """LM head on the loss rows: forward, loss (+ d loss / d logits), backward down to the text rows' gradient st.dh."""
        dev, hd, n = self.dev, self.cls_head, st.n
        hrows = ops.cast_bf16(st.text_out.index_select(0, st.sel).contiguous())
        zt = torch.empty(n, 768, device=dev, dtype=torch.bfloat16)
        gt = ops.gemm_ex(hrows, hd.t.w, bias=hd.t.b, act=L.ACT_GELU_ERF, zout=zt, out_dtype=torch.float32)
        h2b, _ = ops.layernorm(gt, hd.n.g, hd.n.b, 1e-12)
        cbias = torch.zeros(L.VOCAB_PAD, device=dev)
        cbias[:L.VOCAB] = hd.dec.b
        logits = ops.gemm_bias_act(h2b, hd.dec.w, cbias, out_dtype=torch.float32)
        dlog = torch.empty(n, L.VOCAB_PAD, device=dev, dtype=torch.bfloat16)
        check(lib.vitcap_ls_kl_loss(_p(logits), L.VOCAB_PAD, L.VOCAB, _p(st.tgt), 0.0 if st.scst else self.eps_ls, n, _p(st.row_w),
                                    _p(self.loss_buf), _p(dlog), L.VOCAB_PAD, _s()), 'ls_kl')
        bsum = torch.zeros(L.VOCAB_PAD, device=dev)
        dlT = ops.transpose_colsum(dlog, bsum)                                 # [VOCAB_PAD][n_pad]
        hd.dec.gb.copy_(bsum[:L.VOCAB])
        h2T = ops.transpose_colsum(h2b)
        gdec = torch.empty(L.VOCAB_PAD, 768, device=dev)
        ops.gemm_ex(dlT, h2T, out=gdec)
        hd.dec.gw.copy_(gdec[:L.VOCAB])                                        # first writer of the (tied) embedding gradient
        dh2 = ops.gemm_ex(dlog, hd.dec.wt)                                     # [n,768] bf16
        dgt, _ = self._ln_bwd(gt, dh2, hd.n, 1e-12)
        dzt = torch.empty(n, 768, device=dev, dtype=torch.bfloat16)
        check(lib.vitcap_gelu_bwd(_p(dgt), _p(zt), _p(dzt), n * 768, _s()), 'gelu_bwd')
        self._wgrad_tn(dzt, hrows, hd.t.gw, hd.t.gb)
        st.dh = ops.gemm_ex(dzt, hd.t.wt, out_dtype=torch.float32)            # [n,768] fp32

    def _decoder_bwd(self, st):
        """Yields dec1, dec0; leaves the gradient of the decoder's input rows in st.dyv (B, LR, 768)."""
        B, TT = st.B, st.TT
        dtext = torch.zeros(B * TT + 1, 768, device=self.dev)            # + the dummy row unused loss slots write to
        dtext.index_copy_(0, st.sel_bwd, st.dh)
        dtext = dtext[:B * TT]
        dy = dtext if st.prune else self._all_rows(st, dtext)           # pruned: the last layer's backward runs on the text rows
        for l in (3, 2, 1, 0):
            dy = self._dec_bwd(st, l, dy, text_only=(l == 3 and st.prune))
            if l % 2 == 0:
                yield 'dec%d' % (l // 2)
        st.dyv = dy.view(B, st.LR, 768)

    def _embedding_bwd(self, st):
        emb, B, TT = self.emb, st.B, st.TT
        dtext_in = st.dyv[:, SV:].reshape(B * TT, 768).contiguous()
        if st.ph > 0:
            ops.hidden_dropout(dtext_in, None, TT, SV, st.hseed(4, 3), st.ph, out=dtext_in)
        demb, _ = self._ln_bwd(st.pre_emb, dtext_in, emb.n, 1e-12, dres=None)
        check(lib.vitcap_embed_bwd(_p(demb), _p(st.ids20.view(-1)), TT, _p(emb.gword), _p(emb.gpos), _p(emb.gtype),
                                   B * TT, T if st.scst else 0, _s()), 'embed_bwd')

    def _encoder_bwd(self, st):
        """Yields tag1, tag0, blk5 .. blk0; leaves the gradient of the patch embedding's output in st.dxe."""
        Be, KS, M = st.Be, st.KS, st.M
        if KS > 1:      # the KS sequences of an image saw the same visual rows: their gradients add up
            dyv_vis = st.dyv[:, :SV].reshape(Be, KS, SV, 768).sum(1)
        else:
            dyv_vis = st.dyv[:, :SV]
        dhid = dyv_vis[:, 1:SV].reshape(M, 768).contiguous()
        if not st.prune:
            dtag = torch.zeros(Be, NV, 768, device=self.dev)
            dtag[:, 0] = dyv_vis[:, 0]
            dtag = dtag.view(M, 768)
        for i in (3, 2, 1, 0):
            if i == 3 and st.prune:
                dtag = self._vit_bwd(st, self.tag_blocks[3], dyv_vis[:, 0].contiguous(), cls_only=True)
            else:
                dtag = self._vit_bwd(st, self.tag_blocks[i], dtag)
            if i % 2 == 0:
                yield 'tag%d' % (i // 2)
        for i in (11, 10, 9, 8):
            dhid = self._vit_bwd(st, self.blocks[i], dhid)
            if i % 2 == 0:
                yield 'blk%d' % (i // 2)
        dxe = dhid
        ops.reduce_slabs(dtag.view(1, M * 768), dxe.view(-1), accumulate=True)      # fork point: the two branches' gradients meet
        for i in range(7, -1, -1):
            dxe = self._vit_bwd(st, self.blocks[i], dxe)
            if i % 2 == 0:
                yield 'blk%d' % (i // 2)
        st.dxe = dxe

    def _patch_bwd(self, st):
        """Patch embed, cls token, position embedding."""
        Be, dxe = st.Be, st.dxe
        check(lib.vitcap_sum_over_batch(_p(dxe), NV * 768, Be, _p(self.pos_embed.g), NV * 768, _s()), 'sum_over_batch')
        self.cls_token.g.copy_(self.pos_embed.g[0])
        dpatch = ops.cast_bf16(dxe.view(Be, NV, 768)[:, 1:].reshape(Be * 576, 768).contiguous())
        self._wgrad_tn(dpatch, st.patches, self.patch.gw, self.patch.gb)

    # ------------------------------------------------------------------ optimizer
    def all_reduce_grads(self):
        """Joins the bucketed all-reduces that forward_backward launched behind the backward pass (mean over ranks)."""
        self.reducer.finish()

    def optimizer_step(self):
        self.step_no += 1
        self.gsumsq.zero_()
        check(lib.vitcap_sumsq(_p(self.G), self.nflat, _p(self.gsumsq), _s()), 'sumsq')
        self._watch_nan()
        check(lib.vitcap_adamw_multi(_p(self.P), _p(self.G), _p(self.M), _p(self.V), _p(self.chunk_lr), _p(self.chunk_wd),
                                     _p(self.gsumsq), self.clip, self.lr_scale, self.step_no, 0.9, 0.999, 1e-8,
                                     self.nflat // CH, _s()), 'adamw')
        self.lr_scale = max(0.0, float(self.max_iter - self.step_no) / float(max(1.0, self.max_iter)))   # WarmupLinearSchedule
        self.refresh_weights()

    def train_step(self, batch):
        if self.use_graphs and self._graphable(batch):
            return self.train_step_graph(batch)
        loss, tag_loss = self.forward_backward(batch)
        self.all_reduce_grads()
        self.optimizer_step()
        if self.step_no % 50 == 0:
            self.flush_nan_check()
        return {'masked_loss': loss, 'tag_loss': tag_loss}

    # ------------------------------------------------------------------ graph mode: the step as a few host calls
    # The eager step issues ~600 ctypes launches + ~150 torch calls from Python (with 8 ranks x (loader processes +
    # launcher) on one host that is the fragile part).  Here the whole forward + backward is recorded ONCE per batch shape into hipGraph
    # segments (torch.cuda.graph: the stream capture also records torch's own small kernels and keeps the step's activations in a
    # private pool) and a step becomes: copy the batch into the static input buffers (5 calls), rewrite the dropout salt (1), replay
    # the segments (1 without a gradient exchange; 4 with one, the buckets of a segment's stages start behind it), clip + AdamW +
    # weight refresh (4).  Same kernels, same arguments, same order as the eager step: bit-identical parameters with dropout off
    # (tests/test_hip_train_e2e.py::test_graph_step_equals_eager); with dropout on the keep decisions of step t are those of
    # seed(step 0) ^ salt(t) -- another stream than the eager step's, equally distributed.
    GRAPH_SEGMENT_ENDS = ('dec0', 'tag0', 'blk3', 'patch')       # with a gradient exchange: 4 segments (cls+dec | emb+tag | blk5-3 | blk2-0+patch)
    _GRAPH_KEYS = ('image', 'input_ids', 'attention_mask', 'masked_pos', 'masked_ids', 'label')

    def _graphable(self, batch):
        return ('sample_ids' not in batch and int(batch.get('seq_per_image', 1)) == 1 and 'masked_pos' in batch and 'masked_ids' in batch
                and all(torch.is_tensor(batch[k]) for k in self._GRAPH_KEYS if k in batch))

    def _graph_build(self, key, batch):
        dev = self.dev
        static = {k: batch[k].to(dev).clone().contiguous() for k in self._GRAPH_KEYS if k in batch}
        salt = torch.zeros(1, dtype=torch.int32, device=dev)
        # one eager pass on the static buffers first: every kernel's launch attributes exist and the caching allocator is warm.  It runs
        # WITHOUT the gradient exchange: a rank that meets a new batch shape -- a ragged last batch, or a batch that stays
        # eager on another rank -- must not issue one more round of collectives than its peers (RCCL would hang); the pass only
        # changes gradients and the loss buffer, both rewritten by the step that follows
        exchange = self.reducer.exchange
        self.reducer.exchange = False
        try:
            self.forward_backward(static)
            self.all_reduce_grads()
        finally:
            self.reducer.exchange = exchange
        torch.cuda.synchronize(dev)
        segs = []
        pool = torch.cuda.graph_pool_handle()
        gen = self._fb_gen(static, capture=True)
        done = False
        last = GRAD_STAGES[-1]
        check(lib.vitcap_set_dropout_salt(C.c_void_p(salt.data_ptr())), 'set_dropout_salt')
        # The grid of a persistent GEMM is fixed when its launch is RECORDED (vitcap_gemm_reserve_cus is read by the launcher, on the
        # host): a replayed segment keeps whatever reservation was set while it was captured.  The first bucket's collective starts
        # behind segment 0, so every later segment is captured with the reducer's CUs left free (captured after finish()
        # had set the reservation back to 0, the graphs froze all-CU grids and the reservation was a no-op in graph mode).
        reserve = self.reducer.reserve_cus if exchange else 0
        try:
            while not done:
                g = torch.cuda.CUDAGraph()
                stages = []
                if reserve and segs:
                    lib.vitcap_gemm_reserve_cus(reserve)
                with torch.cuda.graph(g, pool=pool, capture_error_mode='thread_local'):     # a loader thread may copy meanwhile
                    while True:
                        try:
                            st = next(gen)
                        except StopIteration:
                            done = True
                            break
                        stages.append(st)
                        # the last stage is followed by nothing but the generator's return: it stays in this segment
                        if exchange and st in self.GRAPH_SEGMENT_ENDS and st != last:
                            break
                segs.append((g, stages))
        finally:
            if reserve:
                lib.vitcap_gemm_reserve_cus(0)
            check(lib.vitcap_set_dropout_salt(None), 'set_dropout_salt')
        entry = {'static': static, 'salt': salt, 'segs': segs, 'reserved_cus': reserve}
        self._graphs[key] = entry
        return entry

    def train_step_graph(self, batch):
        key = tuple((k, tuple(batch[k].shape), str(batch[k].dtype)) for k in self._GRAPH_KEYS if k in batch)
        entry = self._graphs.get(key) or self._graph_build(key, batch)
        for k, t in entry['static'].items():
            t.copy_(batch[k], non_blocking=True)
        if self.attn_dropout > 0 or self.hidden_dropout > 0:
            entry['salt'].fill_(mix32(0x85ebca6b, self.step_no) & 0x7fffffff)
        self.reducer.begin()
        for g, stages in entry['segs']:
            g.replay()
            for st in stages:
                self.reducer.stage_done(st)
        self.all_reduce_grads()
        self.optimizer_step()
        if self.step_no % 50 == 0 or not entry.get('checked'):     # the first replay of a shape as well: a bad batch layout is reported at once
            entry['checked'] = True
            self.flush_text_check()
        return {'masked_loss': self.loss_buf[0], 'tag_loss': self.loss_buf[1]}

    def grad_norm(self):
        return float(self.gsumsq.sqrt())
