"""Host helpers for the occlusion maps of ImageCaptioning.occlusion_maps() / score_masked(): which of an image's 578 visual keys a
caption may see.  A mask row has one flag per visual key in the engine's cache order (vitcap_amd.attnmaps: 0 tag cls, 1 encoder cls,
2..577 the 24 x 24 patches row-major), True = visible.  The engine takes it packed: 19 words of 32 bits per caption, bit k & 31 of
word k >> 5 for key k (vitcap_attn_text_grid_masked).  The mask hides visual TOKENS from the caption; it does not hide patches from
the encoder, so a hidden patch has still shaped the tokens of its neighbours.  No GPU is touched here."""
import numpy as np
import torch

from .attnmaps import COL_PATCH0, GRID, N_PATCH, N_VIS

MASK_WORDS = 19      # 608 bits per caption; bits 578..607 are ignored by the kernel
MAX_ROWS = 32        # captions (here: mask variants) per image in one scoring pass


def check_window(window, stride=None):
    """(window, stride) as occlusion_maps takes them -> (window, stride, windows per grid side); anything else is refused by name."""
    if isinstance(window, bool) or int(window) != window or not 1 <= int(window) <= GRID:
        raise ValueError('occlusion: window must be 1..%d patches (got %r)' % (GRID, window))
    window = int(window)
    if stride is None:
        stride = window
    if isinstance(stride, bool) or int(stride) != stride or not 1 <= int(stride) <= window:
        raise ValueError('occlusion: stride must be 1..window=%d (got %r)' % (window, stride))
    stride = int(stride)
    if (GRID - window) % stride != 0:
        raise ValueError('occlusion: (%d - window) %% stride must be 0, the windows have to tile the %d x %d grid exactly (got window=%d, '
                         'stride=%d)' % (GRID, GRID, GRID, window, stride))
    return window, stride, (GRID - window) // stride + 1


def window_masks(window, stride=None, keep_cls=True, keep_only=False):
    """One mask row per window position, row-major over the (gh, gw) window grid -> bool (gh * gw, 578).  Row g hides window g's
    patches and shows the others; with keep_only it shows ONLY window g's patches.  The two cls columns are visible iff keep_cls."""
    window, stride, g = check_window(window, stride)
    inside = torch.zeros((g, g, GRID, GRID), dtype=torch.bool)
    for i in range(g):
        for j in range(g):
            inside[i, j, i * stride:i * stride + window, j * stride:j * stride + window] = True
    inside = inside.reshape(g * g, N_PATCH)
    out = torch.empty((g * g, N_VIS), dtype=torch.bool)
    out[:, :COL_PATCH0] = bool(keep_cls)
    out[:, COL_PATCH0:] = inside if keep_only else ~inside
    return out


def as_visible(visible, rows, keep_cls=True):
    """The `visible` argument of score_masked / generate -> bool (rows, 578): bool or uint8, (rows, 578) in cache order or a
    (rows, 24, 24) patch grid (then both cls columns are visible iff keep_cls).  A wrong shape or dtype is a ValueError."""
    v = torch.as_tensor(visible)
    if v.dtype not in (torch.bool, torch.uint8):
        raise ValueError('visible must be bool or uint8 (got %s)' % (v.dtype,))
    if tuple(v.shape) == (rows, GRID, GRID):
        full = torch.full((rows, N_VIS), bool(keep_cls), dtype=torch.bool)
        full[:, COL_PATCH0:] = v.reshape(rows, N_PATCH).cpu() != 0
        return full
    if tuple(v.shape) != (rows, N_VIS):
        raise ValueError('visible must be (%d, %d) in cache order or a (%d, %d, %d) patch grid (got %s)'
                         % (rows, N_VIS, rows, GRID, GRID, tuple(v.shape)))
    return v.cpu() != 0


def pack_visible(mask):
    """bool / uint8 (rows, 578) -> int32 (rows, 19): bit k & 31 of word k >> 5 is key k; bits 578..607 are clear."""
    m = torch.as_tensor(mask)
    if m.dim() != 2 or m.shape[1] != N_VIS:
        raise ValueError('pack_visible: the mask must be (rows, %d) (got %s)' % (N_VIS, tuple(m.shape)))
    bits = torch.zeros((m.shape[0], MASK_WORDS * 32), dtype=torch.int64)
    bits[:, :N_VIS] = (m.cpu() != 0).to(torch.int64)
    words = (bits.view(-1, MASK_WORDS, 32) << torch.arange(32, dtype=torch.int64)).sum(-1)      # 0 .. 2^32 - 1
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words)                                 # the same 32 bits as int32
    return words.to(torch.int32)


def upsample(drop, window, stride=None):
    """(B, L, gh, gw) window drops -> (B, L, 24, 24): at every patch the mean of the drops of the windows that cover it."""
    window, stride, g = check_window(window, stride)
    d = torch.as_tensor(drop)
    if d.dim() != 4 or tuple(d.shape[2:]) != (g, g):
        raise ValueError('upsample: drop must be (B, L, %d, %d) at window=%d, stride=%d (got %s)' % (g, g, window, stride, tuple(d.shape)))
    total = torch.zeros(tuple(d.shape[:2]) + (GRID, GRID), dtype=d.dtype, device=d.device)
    count = torch.zeros((GRID, GRID), dtype=d.dtype, device=d.device)
    for i in range(g):
        for j in range(g):
            total[:, :, i * stride:i * stride + window, j * stride:j * stride + window] += d[:, :, i:i + 1, j:j + 1]
            count[i * stride:i * stride + window, j * stride:j * stride + window] += 1
    return total / count


def to_rows(ids, drop, tokenizer, eos=(102,)):
    """One list per image for the occlusion TSV: for every live position of the caption (1 .. the first end token) the word and its
    (gh, gw) drops.  ids (B, L) or (B, 1, L), drop (B, L, gh, gw)."""
    vocab = tokenizer.ids_to_tokens
    ids = torch.as_tensor(ids).reshape(drop.shape[0], -1).tolist()
    grids = np.asarray(torch.as_tensor(drop).cpu(), dtype=np.float32)
    eos = set(int(e) for e in eos)
    out = []
    for b, toks in enumerate(ids):
        L = len(toks)
        ends = [t for t in range(1, L) if toks[t] in eos]
        n = ends[0] if ends else L - 1
        out.append([{'word': vocab[toks[t]], 'drop': [[float(x) for x in row] for row in grids[b, t]]} for t in range(1, n + 1)])
    return out
