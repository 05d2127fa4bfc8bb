"""Attention-map timing: ImageCaptioning.attention_maps at B images x K captions per image against score(one_pass=True) on the same
captions, and vitcap_attn_probe_maps alone per launch (run on the GPU box).
Usage: python tools/attn_maps_bench.py [B=64] [K list=1,5] [iters=10]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vitcap_amd import ops
from vitcap_amd import weights as W
from vitcap_amd.model import ImageCaptioning

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
KS = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else '1,5').split(',')]
ITERS = int(sys.argv[3]) if len(sys.argv) > 3 else 10


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


m = ImageCaptioning().load_recipe(0).eval()
m.pack('cuda')
img = torch.from_numpy(W.gen_image_batch(B, 1)).cuda().to(torch.bfloat16)
ids, _ = m.generate(img)
L = ids.shape[-1]
for K in KS:
    caps = ids[:, 0].repeat_interleave(K, 0).clone()
    for k in range(1, K):                       # the K captions of an image differ in one word each
        caps[k::K, 1 + k % 18] = 2000 + k
    print('B=%d K=%d: score one pass %.2f ms per call' % (B, K, timed(lambda: m.score(img, caps, seqs_per_image=K, one_pass=True))))
    for per_head, layers, name in ((False, (0, 1, 2, 3), 'head mean, all layers'), (False, (3,), 'head mean, last layer'),
                                   (True, (3,), 'per head, last layer')):
        ms = timed(lambda: m.attention_maps(img, caps, seqs_per_image=K, per_head=per_head, layers=layers))
        print('B=%d K=%d: attention_maps %s %.2f ms per call (the zeroed output array included)' % (B, K, name, ms))
    # the kernel alone, on random qkv of the same shapes
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn((B * K * (2 * L - 1), 2304), generator=g).to(torch.bfloat16).cuda()
    vis = torch.randn((B * 578, 2304), generator=g).to(torch.bfloat16).cuda()
    capd = caps.cuda()
    for per_head in (False, True):
        out = torch.zeros((B * K, L, 4) + ((12, 578 + L) if per_head else (578 + L,)), dtype=torch.float32, device='cuda')
        ms = timed(lambda: ops.attn_probe_maps(qkv, vis, capd, B, K, max_len=L, per_head=per_head, layer=0, out=out))
        print('B=%d K=%d: vitcap_attn_probe_maps %s %.3f ms per launch' % (B, K, 'per head' if per_head else 'head mean', ms))
