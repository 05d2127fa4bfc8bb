"""Host helpers for region captions (ImageCaptioning.caption_regions / generate(visible=)): which of an image's 578 visual keys the
caption of a region may see.  A region is a box [row0, col0, row1, col1) on the 24 x 24 patch grid (half-open, in patches of 16 x 16
pixels of the 384 x 384 input) or a (24, 24) bool grid; its mask row shows the region's patches and hides every other patch, and the
two cls columns are visible iff keep_cls (vitcap_amd.attnmaps: 0 tag cls, 1 encoder cls, 2..577 the patches row-major).  The engine
takes the rows packed by vitcap_amd.occlusion.pack_visible.  The mask hides visual TOKENS from the caption; it does not hide patches
from the encoder, so a hidden patch has still shaped the tokens of its neighbours and the cls tokens.  No GPU is touched here."""
import math

import torch

from .attnmaps import COL_PATCH0, GRID, N_PATCH, N_VIS

PATCH = 16           # pixels per patch side
MAX_REGIONS = 8      # regions of an image in one decode pass (vitcap_gen_opts.seqs_per_image)


def check_boxes(boxes):
    """Integer boxes (..., 4) as [row0, col0, row1, col1) -> int64 tensor; a wrong shape or dtype, an empty box or one that leaves
    the grid is refused by name."""
    b = torch.as_tensor(boxes)
    if b.dim() < 1 or b.shape[-1] != 4 or b.numel() == 0:
        raise ValueError('regions: boxes must be (..., 4) as [row0, col0, row1, col1) (got shape %s)' % (tuple(b.shape),))
    if b.dtype in (torch.bool, torch.float16, torch.bfloat16, torch.float32, torch.float64):
        raise ValueError('regions: boxes must be integers, in patches of the %d x %d grid (got %s)' % (GRID, GRID, b.dtype))
    b = b.to(torch.int64).cpu()
    r0, c0, r1, c1 = b.unbind(-1)
    if bool(((r1 <= r0) | (c1 <= c0)).any()):
        raise ValueError('regions: empty box (row1 <= row0 or col1 <= col0); boxes are half-open [row0, col0, row1, col1)')
    if bool(((r0 < 0) | (c0 < 0) | (r1 > GRID) | (c1 > GRID)).any()):
        raise ValueError('regions: box outside the %d x %d patch grid' % (GRID, GRID))
    return b


def box_masks(boxes, keep_cls=True):
    """boxes (R, 4) -> bool (R, 578): row r shows ONLY box r's patches; the two cls columns are visible iff keep_cls."""
    b = check_boxes(boxes)
    if b.dim() != 2:
        raise ValueError('regions: box_masks takes boxes of shape (R, 4) (got %s)' % (tuple(b.shape),))
    rows = torch.arange(GRID).view(1, GRID, 1)
    cols = torch.arange(GRID).view(1, 1, GRID)
    r0, c0, r1, c1 = (x.view(-1, 1, 1) for x in b.unbind(-1))
    inside = (rows >= r0) & (rows < r1) & (cols >= c0) & (cols < c1)
    out = torch.empty((b.shape[0], N_VIS), dtype=torch.bool)
    out[:, :COL_PATCH0] = bool(keep_cls)
    out[:, COL_PATCH0:] = inside.reshape(-1, N_PATCH)
    return out


def grid_regions(g):
    """The g x g tiling of the patch grid, row-major -> int64 (g * g, 4) boxes; g must divide 24."""
    if isinstance(g, bool) or int(g) != g or int(g) < 1 or GRID % int(g) != 0:
        raise ValueError('regions: the tiling g must be a positive divisor of %d (got %r)' % (GRID, g))
    g = int(g)
    s = GRID // g
    return torch.tensor([[i * s, j * s, (i + 1) * s, (j + 1) * s] for i in range(g) for j in range(g)], dtype=torch.int64)


def region_masks(regions, B, keep_cls=True):
    """The `regions` argument of caption_regions -> (bool (B, R, 578), boxes int64 (B, R, 4) or None): integer boxes (B, R, 4) or
    (R, 4) (the same regions for every image), or bool / uint8 grids (B, R, 24, 24)."""
    r = torch.as_tensor(regions)
    if r.dtype in (torch.bool, torch.uint8) and r.dim() == 4:
        if tuple(r.shape[0:1] + r.shape[2:]) != (B, GRID, GRID) or r.shape[1] < 1:
            raise ValueError('regions: grids must be (%d, R, %d, %d) (got %s)' % (B, GRID, GRID, tuple(r.shape)))
        out = torch.full((B, r.shape[1], N_VIS), bool(keep_cls), dtype=torch.bool)
        out[:, :, COL_PATCH0:] = r.reshape(B, r.shape[1], N_PATCH).cpu() != 0
        return out, None
    b = check_boxes(r)
    if b.dim() == 2:
        b = b.unsqueeze(0).expand(B, -1, -1)
    if b.dim() != 3 or b.shape[0] != B:
        raise ValueError('regions: boxes must be (%d, R, 4) or (R, 4), or grids (%d, R, %d, %d) (got %s)'
                         % (B, B, GRID, GRID, tuple(r.shape)))
    R = b.shape[1]
    return box_masks(b.reshape(B * R, 4), keep_cls).view(B, R, N_VIS), b.contiguous()


def to_rows(ids, logprobs, boxes, tokenizer):
    """One list per image for the regions TSV: per region its pixel rectangle [x0, y0, x1, y1) in the 384 x 384 input, the caption
    and its confidence exp(logprob).  ids (B, R, L), logprobs (B, R), boxes (R, 4) or (B, R, 4).
    The n-best shape of caption_regions_beam -- ids (B, R, keep, L), logprobs (B, R, keep), best first: 'caption' and 'conf' are the
    best hypothesis', and with keep > 1 'nbest' lists all of them as {'caption', 'conf'}; a slot the search left empty (fewer than
    keep finished hypotheses: score -1e5) is left out."""
    ids = torch.as_tensor(ids).cpu()
    if ids.dim() == 4:
        keep = ids.shape[2]
        lpk = torch.as_tensor(logprobs).cpu()
        if tuple(lpk.shape) != tuple(ids.shape[:3]):
            raise ValueError('regions: to_rows needs logprobs %s next to n-best ids %s (got %s)'
                             % (tuple(ids.shape[:3]), tuple(ids.shape), tuple(lpk.shape)))
        out = to_rows(ids[:, :, 0], lpk[:, :, 0], boxes, tokenizer)
        if keep > 1:
            for i, recs in enumerate(out):
                for r, rec in enumerate(recs):
                    rec['nbest'] = [{'caption': tokenizer.decode(ids[i, r, k].tolist(), skip_special_tokens=True),
                                     'conf': math.exp(float(lpk[i, r, k]))} for k in range(keep) if float(lpk[i, r, k]) > -1e4]
        return out
    if ids.dim() != 3:
        raise ValueError('regions: to_rows needs ids (B, R, L) or (B, R, keep, L) (got %s)' % (tuple(ids.shape),))
    B, R = ids.shape[0], ids.shape[1]
    lp = torch.as_tensor(logprobs).cpu().reshape(B, R).tolist()
    b = check_boxes(boxes)
    if b.dim() == 2:
        b = b.unsqueeze(0).expand(B, -1, -1)
    if tuple(b.shape) != (B, R, 4):
        raise ValueError('regions: to_rows needs boxes (%d, 4) or (%d, %d, 4) (got %s)' % (R, B, R, tuple(b.shape)))
    out = []
    for i in range(B):
        recs = []
        for r in range(R):
            r0, c0, r1, c1 = (int(x) * PATCH for x in b[i, r].tolist())
            recs.append({'rect': [c0, r0, c1, r1], 'caption': tokenizer.decode(ids[i, r].tolist(), skip_special_tokens=True),
                         'conf': math.exp(lp[i][r])})
        out.append(recs)
    return out
