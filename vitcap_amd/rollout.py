"""Host helpers of the encoder attention rollout (ImageCaptioning.encoder_attention / tag_rollout / rollout_maps /
caption_with_rollout): block selection, chunk sizing, the model's graph walked backwards (rollout_rows) and the rows of the
rollout TSV.

Attention rollout (Abnar & Zuidema 2020) models a block as A~ = r I + (1 - r) A, with A the block's head-mean attention and r I its
residual connection, and the flow of information through a stack of blocks as the product of their A~.  It is a model of flow through
ATTENTION ALONE: the MLPs, the LayerNorms and the value vectors play no part in it.  Here only the rows that are asked for are
carried back through the blocks (one per tagger question, at most max_length per caption); the 577 x 577 product is never formed.
"""
import numpy as np

N_BLOCKS = 16
N_ENC = 577              # the encoder's rows: [cls | 576 patches]
N_VIS = 578              # the decoder's visual tokens: [tag-branch cls | cls | 576 patches]
GRID = 24
FORK = 8                 # blocks[8..11] and tag_blocks[0..3] both read the output of blocks[7] (modeling_bert.py:458-478)
BLOCK_NAMES = tuple('blocks.%d' % i for i in range(12)) + tuple('tag_blocks.%d' % i for i in range(4))
ALL_BLOCKS = (1 << N_BLOCKS) - 1
MAX_ROWS = 64                # rows per image of one vitcap_rollout_step launch
MAX_CALL_BYTES = 1 << 30     # one engine call's maps buffer stays at or below this


def parse_blocks(blocks):
    """`blocks`: None (all 16) or an iterable of ints 0..15 (12..15 = the tag blocks) / names 'blocks.3', 'tag_blocks.0'
    -> (engine bit mask, names of the selected blocks in ascending bit order)."""
    if blocks is None:
        return ALL_BLOCKS, list(BLOCK_NAMES)
    if isinstance(blocks, (str, int)):
        blocks = [blocks]
    mask = 0
    for b in blocks:
        if isinstance(b, str):
            if b not in BLOCK_NAMES:
                raise ValueError('blocks: %r names no encoder block (blocks.0..11, tag_blocks.0..3)' % (b,))
            bit = BLOCK_NAMES.index(b)
        elif isinstance(b, (int, np.integer)) and not isinstance(b, bool):
            bit = int(b)
            if not 0 <= bit < N_BLOCKS:
                raise ValueError('blocks: %r is outside 0..15 (0..11 the blocks, 12..15 the tag blocks)' % (b,))
        else:
            raise ValueError('blocks: %r is neither a block index nor a block name' % (b,))
        mask |= 1 << bit
    if mask == 0:
        raise ValueError('blocks: at least one block must be selected')
    return mask, [BLOCK_NAMES[i] for i in range(N_BLOCKS) if mask >> i & 1]


def maps_bytes(n_images, n_sel, per_head):
    """Bytes of the fp32 maps of one engine call."""
    return int(n_images) * int(n_sel) * (12 if per_head else 1) * N_ENC * N_ENC * 4


def images_per_call(n_sel, per_head, limit=MAX_CALL_BYTES):
    """Images one engine call may cover so that its maps stay at or below `limit` bytes (at least one: a single image's per-head
    maps of all 16 blocks are 256 MB)."""
    return max(1, int(limit) // maps_bytes(1, n_sel, per_head))


def check_residual(residual):
    r = float(residual)
    if not 0.0 <= r <= 1.0:          # also refuses NaN
        raise ValueError('residual must be in [0, 1] (got %r)' % (residual,))
    return r


def rollout_rows(A, w, residual=0.5):
    """The model's graph, walked backwards.  A: fp32 device tensor (16, n_img, 577, 577), the head-mean attention of the 16 blocks in
    BLOCK_NAMES order (what encoder_attention returns for blocks=None); w: (n_img, rows, 578), weights over the decoder's visual
    tokens in cache order [tag-branch cls | cls | 576 patches].
      1. v_cap = w[..., 1:] goes back through blocks 11, 10, 9, 8;
      2. v_tag = w[..., 0] e_0 goes back through tag blocks 3 (whose matrix holds its cls row only), 2, 1, 0;
      3. v_cap + v_tag goes back through blocks 7 .. 0.
    -> (n_img, rows, 577) over the encoder's inputs [cls | 576 patches].  Every step is one vitcap_rollout_step launch (fp32, fixed
    order); the split and the sum are torch plumbing.  Every step's matrix is row-stochastic, so row sums are conserved."""
    import torch
    from . import ops
    r = check_residual(residual)
    if A.dim() != 4 or tuple(A.shape[::2]) != (N_BLOCKS, N_ENC) or A.shape[3] != N_ENC:
        raise ValueError('rollout_rows: A must be (16, n_img, 577, 577), got %s' % (tuple(A.shape),))
    n_img = A.shape[1]
    if w.dim() != 3 or w.shape[0] != n_img or w.shape[2] != N_VIS:
        raise ValueError('rollout_rows: w must be (%d, rows, 578), got %s' % (n_img, tuple(w.shape)))
    w = w.to(device=A.device, dtype=torch.float32)
    A = A.contiguous()
    if w.shape[1] > MAX_ROWS:          # vitcap_rollout_step carries at most 64 rows per image
        return torch.cat([rollout_rows(A, w[:, i:i + MAX_ROWS], r) for i in range(0, w.shape[1], MAX_ROWS)], 1)
    v = w[..., 1:].contiguous()
    for b in range(11, FORK - 1, -1):
        v = ops.rollout_step(v, A[b], r)
    t = torch.zeros_like(v)
    t[..., 0] = w[..., 0]
    for b in range(15, 11, -1):
        t = ops.rollout_step(t, A[b], r)
    v = v + t
    for b in range(FORK - 1, -1, -1):
        v = ops.rollout_step(v, A[b], r)
    return v


def patch_grid(v):
    """(..., 577) rollout rows -> ((..., 24, 24) patch map, (...) mass left on the encoder's cls input)."""
    if v.shape[-1] != N_ENC:
        raise ValueError('patch_grid: the last dimension is %d, a rollout row has %d entries' % (v.shape[-1], N_ENC))
    return v[..., 1:].reshape(tuple(v.shape[:-1]) + (GRID, GRID)), v[..., 0]


def to_rows(tokens, tag_map, word_maps):
    """The JSON record of one image in the rollout TSV, in the encoding of the attention TSV: float16, row-major, base64.  Map 0 is
    the tag head's (24, 24), map 1 + i that of live word i of the caption (tokens[i]); word_maps (n, 24, 24)."""
    import base64
    tag = np.asarray(tag_map, dtype=np.float32).reshape(1, GRID, GRID)
    words = np.asarray(word_maps, dtype=np.float32).reshape(len(tokens), GRID, GRID)
    data = np.ascontiguousarray(np.concatenate([tag, words], 0).astype(np.float16))
    return {'tokens': list(tokens), 'first': 'tag', 'shape': list(data.shape), 'dtype': 'float16',
            'data': base64.b64encode(data.tobytes()).decode('ascii')}


def from_rows(rec):
    """The inverse of to_rows -> (tokens, tag map float16 (24, 24), word maps float16 (n, 24, 24))."""
    import base64
    if rec.get('dtype') != 'float16' or list(rec['shape'])[1:] != [GRID, GRID] or rec['shape'][0] != len(rec['tokens']) + 1:
        raise ValueError('from_rows: not a rollout record (dtype %r, shape %r, %d tokens)' % (rec.get('dtype'), rec.get('shape'), len(rec['tokens'])))
    data = np.frombuffer(base64.b64decode(rec['data']), dtype=np.float16).reshape(rec['shape'])
    return rec['tokens'], data[0], data[1:]
