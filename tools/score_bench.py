"""Scoring throughput: captions/s of ImageCaptioning.score at B images x K captions per image (run on the GPU box).
Usage: python tools/score_bench.py [B=64] [K list=1,5] [iters=10] [paths=both|stepwise|one_pass]
Both paths are timed in one run by default: the stepwise forced decode loop (K <= 8) and the one-pass scorer (K <= 32)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vitcap_amd import weights as W
from vitcap_amd.model import ImageCaptioning

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
KS = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else '1,5').split(',')]
ITERS = int(sys.argv[3]) if len(sys.argv) > 3 else 10
PATHS = sys.argv[4] if len(sys.argv) > 4 else 'both'
assert PATHS in ('both', 'stepwise', 'one_pass'), PATHS

m = ImageCaptioning().load_recipe(0).eval()
m.pack('cuda')
img = torch.from_numpy(W.gen_image_batch(B, 1)).cuda().to(torch.bfloat16)
ids, _ = m.generate(img)
for K in KS:
    caps = ids[:, 0].repeat_interleave(K, 0).clone()
    for k in range(1, K):                       # the K captions of an image differ in one word each
        caps[k::K, 1 + k % 18] = 2000 + k
    for one_pass in (False, True):
        if PATHS != 'both' and one_pass != (PATHS == 'one_pass'):
            continue
        if not one_pass and K > 8:              # the stepwise path takes at most 8 captions per image
            continue
        fn = lambda: m.score(img, caps, seqs_per_image=K, one_pass=one_pass)
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / ITERS
        print('score %s B=%d K=%d: %.2f ms per call, %.0f captions/s (%.0f images/s)'
              % ('one pass' if one_pass else 'stepwise', B, K, ms, B * K / ms * 1e3, B / ms * 1e3))
