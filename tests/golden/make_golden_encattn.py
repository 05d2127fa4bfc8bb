"""Golden encoder attention: the reference's `attn` of every ViT block and its fp64 rollout (container only).

Run:  python tests/golden/make_golden_encattn.py      (writes tests/golden/reference_encattn.npz, data only)

Imports the reference model with the shims of make_golden.py, loads the seeded recipe weights (seed 0, tied weights, tagemb = cls)
and runs the reference's own greedy ViTCAP.generate on gen_image_batch(2, 1234).  Forward pre-hooks on the attention-dropout module
of all 12 + 4 blocks (Attention.attn_drop, whose input is `attn` after its softmax, vision_transformer.py:179-183) capture the
(B, 12, 577, 577) probabilities of the encoder pass (the reference repeats that pass at every decode step; the script asserts
that the repeats are identical and keeps the first).

Stored:
    mean          (16, 2, 3, 577)  head-mean query rows {0, 289, 576} of blocks.0..11, tag_blocks.0..3, both images
    per_head      (3, 12, 577)     per-head row 0 of blocks.0, blocks.11, tag_blocks.3, image 0
    tag_rollout   (2, 577)         fp64 rollout (residual 0.5) of e_0 = the tag branch's cls along tag blocks 3..0, blocks 7..0
    cls_rollout   (2, 577)         fp64 rollout of e_cls = the caption branch's cls along blocks 11..0
both computed here from the reference's full head-mean matrices with numpy matrix products, A~ = 0.5 I + 0.5 A per block.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import install_shims, build_reference, load_recipe, ref_generate, REPO  # noqa: E402

ROWS = (0, 289, 576)
PH_BLOCKS = (0, 11, 15)
RESIDUAL = 0.5


def rollout(mats, order, start):
    """e_start through the blocks of `order` (last block first): row vector times A~ of each, fp64."""
    v = np.zeros((mats[0].shape[0], 577))
    v[:, start] = 1.0
    for b in order:
        v = RESIDUAL * v + (1.0 - RESIDUAL) * np.einsum('bj,bjk->bk', v, mats[b])
    return v


def main():
    install_shims()
    sys.path.insert(0, REPO)
    from vitcap_amd import weights as Wt
    torch.manual_seed(0)
    torch.set_num_threads(8)
    model, enc = build_reference('cls', True)
    load_recipe(model, enc, Wt.make_state_dict(seed=0, tie_weights=True))
    img = torch.from_numpy(Wt.gen_image_batch(2, 1234))

    blocks = list(model.bert.encoder.blocks) + list(model.bert.encoder.tag_blocks)
    assert len(blocks) == 16
    got = [[] for _ in blocks]
    hooks = [b.attn.attn_drop.register_forward_pre_hook(lambda m, inp, i=i: got[i].append(inp[0].detach().clone()))
             for i, b in enumerate(blocks)]
    ids, lp, _ = ref_generate(model, enc, img)
    for h in hooks:
        h.remove()
    # ViTCAP.generate runs the whole model, encoder included, at every step on the same image: every pass repeats the first
    assert all(len(g) == len(got[0]) >= 1 for g in got), [len(g) for g in got]
    assert all(torch.equal(a, g[0]) for g in got for a in g[1:])
    attn = [g[0] for g in got]
    assert all(tuple(a.shape) == (2, 12, 577, 577) for a in attn)
    gold = np.load(os.path.join(HERE, 'reference_vectors.npz'))
    assert (ids[:, 0].numpy() == gold['greedy_b2_ids'][:, 0]).all()

    full = [a.double().mean(1).numpy() for a in attn]                      # (2, 577, 577) fp64 per block
    mean = np.stack([m[:, list(ROWS)] for m in full]).astype(np.float32)
    per_head = np.stack([attn[b][0, :, 0].numpy() for b in PH_BLOCKS]).astype(np.float32)
    tag_ro = rollout(full, [15, 14, 13, 12, 7, 6, 5, 4, 3, 2, 1, 0], 0)
    cls_ro = rollout(full, [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0], 0)
    out = {'torch_version': np.array(torch.__version__), 'image_seed': np.array(1234), 'rows': np.array(ROWS), 'mean': mean,
           'per_head_blocks': np.array(PH_BLOCKS), 'per_head': per_head, 'residual': np.array(RESIDUAL),
           'tag_rollout': tag_ro, 'cls_rollout': cls_ro}
    path = os.path.join(HERE, 'reference_encattn.npz')
    np.savez_compressed(path, **out)
    print('row sums', mean.sum(-1).min(), mean.sum(-1).max(), 'rollout sums', tag_ro.sum(-1), cls_ro.sum(-1))
    print('tag rollout / uniform', (tag_ro.min() * 577).round(3), (tag_ro.max() * 577).round(3))
    print('tag vs cls path', float(np.abs(tag_ro - cls_ro).max() / cls_ro.max()))
    print('bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
