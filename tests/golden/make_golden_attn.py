"""Golden attention maps: the reference's attention_probs of the [MASK] row at chosen decode steps (container only).

Run:  python tests/golden/make_golden_attn.py      (writes tests/golden/reference_attn.npz, data only)

Imports the reference model with the shims of make_golden.py, loads the seeded recipe weights and runs the reference's own greedy
ViTCAP.generate on the seeded images (make_golden.py's ref_generate, B = 2).  Forward pre-hooks on the four decoder layers'
attention-dropout modules (BertSelfAttention.dropout, whose input is attention_probs, modeling_bert.py:320-342) capture the
probabilities of every step.  ViTCAP.generate runs every step on the whole sequence so far (prepare_inputs_for_generation with
past = None, modeling_bert.py:845-876), so step t (cur_len = t) has t + 1 + 50 + 578 rows and keys and the [MASK] is query row t.
That row is kept and reordered to the width-W layout of include/vitcap_hip.h (vitcap_attn_probe_maps), W = 578 + 20:

    step t keys  [tokens 0..t-1, MASK, 50 tags, 578 visual]
    stored row   [578 visual | tokens 0..t-1 | MASK | zeros]

The 50 tag columns are masked with -10000, which underflows to exactly 0 in the fp32 softmax; this script asserts it and stores the
largest tag mass it saw (0.0).  Stored: head mean for 2 images x steps {1, 5, 10, 19} x 4 layers, per head for image 0 x steps
{1, 19} x layers {0, 3}, the captions' ids, torch.__version__.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import install_shims, build_reference, load_recipe, ref_generate, REPO  # noqa: E402

L, NVIS, NTAG = 20, 578, 50
W = NVIS + L
STEPS = (1, 5, 10, 19)
PH_STEPS, PH_LAYERS = (1, 19), (0, 3)


def to_layout(row, t):
    """attention_probs[b, h, MASK row, :] of step t -> ((..., W) row, tag mass)."""
    out = torch.zeros(row.shape[:-1] + (W,), dtype=row.dtype)
    assert row.shape[-1] == t + 1 + NTAG + NVIS
    out[..., :NVIS] = row[..., t + 1 + NTAG:]
    out[..., NVIS:NVIS + t + 1] = row[..., :t + 1]
    tags = row[..., t + 1:t + 1 + NTAG]
    return out, float(tags.abs().max())


def main():
    install_shims()
    sys.path.insert(0, REPO)
    from vitcap_amd import weights as Wt
    torch.manual_seed(0)
    torch.set_num_threads(8)
    model, enc = build_reference('cls', True)
    load_recipe(model, enc, Wt.make_state_dict(seed=0, tie_weights=True))
    img = torch.from_numpy(Wt.gen_image_batch(2, 1234))

    calls = [[] for _ in range(4)]          # per layer: the [MASK] row of attention_probs of every step, in call order
    hooks = []

    def keep(l, probs):                     # (B, 12, S, S) with S = t + 1 + 50 + 578: step t, the [MASK] is query row t
        t = probs.shape[-1] - (1 + NTAG + NVIS)
        assert probs.shape[-2] == probs.shape[-1] and t == len(calls[l]) + 1
        calls[l].append(probs[:, :, t, :].detach().clone())

    for l in range(4):
        drop = model.bert.decoder.layer[l].attention.self.dropout
        hooks.append(drop.register_forward_pre_hook(lambda m, inp, l=l: keep(l, inp[0])))
    ids, lp, _ = ref_generate(model, enc, img)
    for h in hooks:
        h.remove()
    n_steps = len(calls[0])
    assert all(len(c) == n_steps for c in calls) and n_steps >= max(STEPS), n_steps
    ids = ids[:, 0]
    print('ids', ids.tolist(), 'steps run', n_steps)

    mean = np.zeros((2, len(STEPS), 4, W), np.float32)
    per_head = np.zeros((len(PH_STEPS), len(PH_LAYERS), 12, W), np.float32)
    tag_mass = 0.0
    for si, t in enumerate(STEPS):
        for l in range(4):
            probs = calls[l][t - 1]                      # (B, 12, keys)
            assert probs.shape[0] == 2 and probs.shape[1] == 12
            rows, tm = to_layout(probs, t)               # (B, 12, W)
            tag_mass = max(tag_mass, tm)
            mean[:, si, l] = rows.double().mean(1).float().numpy()
            if t in PH_STEPS and l in PH_LAYERS:
                per_head[PH_STEPS.index(t), PH_LAYERS.index(l)] = rows[0].numpy()
    assert tag_mass == 0.0, tag_mass
    gold = np.load(os.path.join(HERE, 'reference_vectors.npz'))
    assert (ids.numpy() == gold['greedy_b2_ids'][:, 0]).all()
    out = {'torch_version': np.array(torch.__version__), 'image_seed': np.array(1234), 'ids': ids.numpy().copy(),
           'logprobs': lp.numpy().copy(), 'steps': np.array(STEPS), 'mean': mean, 'per_head_steps': np.array(PH_STEPS),
           'per_head_layers': np.array(PH_LAYERS), 'per_head': per_head, 'tag_mass': np.array(tag_mass)}
    path = os.path.join(HERE, 'reference_attn.npz')
    np.savez_compressed(path, **out)
    print('row sums', mean.sum(-1).min(), mean.sum(-1).max(), 'text mass', mean[..., NVIS:].sum(-1).round(3).tolist())
    print('max / uniform per row', (mean.max(-1) * W).round(2).tolist())
    print('bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
