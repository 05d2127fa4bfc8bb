"""Dense attention with keys removed (vitcap_attn_dense_fwd_keys) against the plain kernel: us per launch at the encoder's shape
(B images x 12 heads, S = 577, bit0 = 1), back-to-back launches, the four arms interleaved over the rounds:
  plain; KEYMASK with every key visible; with all patches but a 6 x 6 box removed (4 of the 10 key tiles live);
  with the lower half of the image removed (5 of 10 live).
    python tools/attn_keys_time.py [B] [rounds]        (run from a tree's root: imports that tree's vitcap_amd)"""
import os, sys
sys.path.insert(0, os.getcwd())
import torch
from vitcap_amd import ops
from vitcap_amd.occlusion import pack_visible
from vitcap_amd.regions import box_masks
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
S, N = 577, 200
qkv = (torch.randn(B * S, 2304, device='cuda') * 0.5).to(torch.bfloat16)
allv = torch.ones(1, 578, dtype=torch.bool)
box = box_masks(torch.tensor([[9, 9, 15, 15]]))
half = allv.clone()
half[:, 2 + 12 * 24:] = False
arms = [('plain', None)] + [(n, pack_visible(m).repeat(B, 1).cuda().contiguous()) for n, m in (('keys, all visible', allv), ('keys, 6 x 6 box', box),
                                                                                              ('keys, upper half', half))]
live = {n: None if m is None else sorted({(k - 1) // 64 for k in range(1, 578) if (int(m[0, k >> 5]) >> (k & 31)) & 1}) for n, m in arms}


def launch(m):
    return ops.attn_dense(qkv, B, S) if m is None else ops.attn_dense_keys(qkv, B, S, m, bit0=1)


for _, m in arms:
    for _ in range(5):
        launch(m)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
times = {n: [] for n, _ in arms}
for rep in range(rounds):
    for n, m in arms:
        e0.record()
        for _ in range(N):
            launch(m)
        e1.record()
        torch.cuda.synchronize()
        times[n].append(e0.elapsed_time(e1) / N * 1e3)
same = torch.equal(launch(None).view(torch.int16), launch(arms[1][1]).view(torch.int16))
for n, _ in arms:
    t = sorted(times[n])
    tiles = '' if live[n] is None else '; live key tiles %s%s' % ([i for i in live[n] if i < S // 64], ' + the left-over key' if S // 64 in live[n] else '')
    print('B=%d S=%d %-18s: median %.1f us per launch (min %.1f, max %.1f over %d rounds)%s' % (B, S, n, t[len(t) // 2], t[0], t[-1], rounds, tiles))
print('all-visible output equals the plain kernel bit for bit:', same)
