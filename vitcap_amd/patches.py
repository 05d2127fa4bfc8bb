"""Host helpers for patch removal (ImageCaptioning.tag_patches / caption_patches / score_patches / caption_crops): which of an image's
576 patches are PRESENT.  An absent patch is removed as a key from every attention row of the model -- all 12 + 4 ViT blocks, the
decoder's visual rows and the caption rows -- so the tagger and the caption see the image without it; unlike the visibility masks of
vitcap_amd.occlusion / vitcap_amd.regions, which hide visual tokens from the caption only after the encoder has seen the whole image.
The two cls keys are always present.  The engine takes one row of 19 words per image in cache order (vitcap_amd.attnmaps: 0 tag cls,
1 encoder cls, 2..577 the 24 x 24 patches row-major), packed by vitcap_amd.occlusion.pack_visible.  No GPU is touched here."""
import math

import torch

from .attnmaps import COL_PATCH0, GRID, N_PATCH, N_VIS
from .occlusion import pack_visible
from .regions import PATCH, check_boxes, region_masks

MAX_CROPS = 32       # (image, region) pairs encoded in one pass of caption_crops


def as_present(present, B):
    """The `present` argument -> bool (B, 578) in cache order with both cls keys set: bool or uint8, a (B, 24, 24) patch grid or
    (B, 576) row-major.  A (B, 578) form is taken too, but one that clears bit 0 or 1 is refused: the cls keys cannot be removed."""
    v = torch.as_tensor(present)
    if v.dtype not in (torch.bool, torch.uint8):
        raise ValueError('present must be bool or uint8 (got %s)' % (v.dtype,))
    v = v.cpu() != 0
    if tuple(v.shape) == (B, N_VIS):
        if not bool(v[:, :COL_PATCH0].all()):
            raise ValueError('present: the two cls keys (columns 0 and 1 of the (B, 578) form) are always present and cannot be removed')
        return v.clone()
    if tuple(v.shape) not in ((B, GRID, GRID), (B, N_PATCH)):
        raise ValueError('present must be (%d, %d, %d) or (%d, %d) (got %s)' % (B, GRID, GRID, B, N_PATCH, tuple(v.shape)))
    full = torch.ones((B, N_VIS), dtype=torch.bool)
    full[:, COL_PATCH0:] = v.reshape(B, N_PATCH)
    return full


def pack_present(present, B):
    """`present` -> int32 (B, 19), the words vitcap_engine_encode_patches reads (and, as vis_mask, every call behind it)."""
    return pack_visible(as_present(present, B))


def crop_masks(regions, B=1):
    """`regions` as caption_regions takes them (integer boxes (R, 4) / (B, R, 4) as [row0, col0, row1, col1), or bool grids
    (B, R, 24, 24)) -> (present bool (B, R, 24, 24): only the region's patches, boxes int64 (B, R, 4) or None)."""
    masks, boxes = region_masks(regions, B, True)
    return masks[:, :, COL_PATCH0:].reshape(B, masks.shape[1], GRID, GRID), boxes


def to_rows(ids, logprobs, tag_topk, tag_prob, boxes, tokenizer, threshold=0.2):
    """One list per image for the crops TSV: per crop its pixel rectangle [x0, y0, x1, y1) in the 384 x 384 input, the caption with
    its confidence exp(logprob), and the tag words whose probability reaches `threshold` (the reference's tag cut, 0.2), best first.
    ids (B, R, L), logprobs (B, R), tag_topk / tag_prob (B, R, 50), boxes (R, 4) or (B, R, 4)."""
    ids = torch.as_tensor(ids).cpu()
    if ids.dim() != 3:
        raise ValueError('patches: to_rows needs ids (B, R, L) (got %s)' % (tuple(ids.shape),))
    B, R = ids.shape[:2]
    lp = torch.as_tensor(logprobs).cpu().reshape(B, R).tolist()
    tk, tp = torch.as_tensor(tag_topk).cpu(), torch.as_tensor(tag_prob).cpu()
    if tuple(tk.shape[:2]) != (B, R) or tuple(tp.shape) != tuple(tk.shape):
        raise ValueError('patches: to_rows needs tag_topk / tag_prob (%d, %d, k) (got %s / %s)' % (B, R, tuple(tk.shape), tuple(tp.shape)))
    b = check_boxes(boxes)
    if b.dim() == 2:
        b = b.unsqueeze(0).expand(B, -1, -1)
    if tuple(b.shape) != (B, R, 4):
        raise ValueError('patches: to_rows needs boxes (%d, 4) or (%d, %d, 4) (got %s)' % (R, B, R, tuple(b.shape)))
    vocab = tokenizer.ids_to_tokens
    out = []
    for i in range(B):
        recs = []
        for r in range(R):
            r0, c0, r1, c1 = (int(x) * PATCH for x in b[i, r].tolist())
            tags = [{'tag': vocab[int(t)], 'prob': float(p)} for t, p in zip(tk[i, r].tolist(), tp[i, r].tolist()) if p >= threshold]
            recs.append({'rect': [c0, r0, c1, r1], 'caption': tokenizer.decode(ids[i, r].tolist(), skip_special_tokens=True),
                         'conf': math.exp(lp[i][r]), 'tags': tags})
        out.append(recs)
    return out
