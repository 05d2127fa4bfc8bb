"""Encoder-rollout timing: ImageCaptioning.tag_rollout and rollout_maps at B images x K captions per image next to generate() and
attention_maps() on the same inputs, and vitcap_attn_self_maps / vitcap_rollout_step alone per launch (run on the GPU box).
Usage: python tools/rollout_bench.py [B=16] [K list=1,5] [iters=10]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vitcap_amd import ops
from vitcap_amd import weights as W
from vitcap_amd.model import ImageCaptioning

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
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
print('B=%d: generate %.2f ms per call' % (B, timed(lambda: m.generate(img))))
print('B=%d: tag_rollout %.2f ms per call' % (B, timed(lambda: m.tag_rollout(img))))
print('B=%d: encoder_attention head mean, all blocks %.2f ms per call' % (B, timed(lambda: m.encoder_attention(img))))
print('B=%d: caption_with_rollout %.2f ms per call' % (B, timed(lambda: m.caption_with_rollout(img))))
for K in KS:
    caps = ids[:, 0].repeat_interleave(K, 0).clone()
    for k in range(1, K):                       # the K captions of an image differ in one word each
        caps[k::K, 1 + k % 18] = 2000 + k
    print('B=%d K=%d: attention_maps head mean, all layers %.2f ms per call' % (B, K, timed(lambda: m.attention_maps(img, caps, seqs_per_image=K))))
    print('B=%d K=%d: rollout_maps %.2f ms per call' % (B, K, timed(lambda: m.rollout_maps(img, caps, seqs_per_image=K))))
# the kernels alone, on random inputs of the encoder's shapes
g = torch.Generator().manual_seed(0)
for b in (1, 16):
    qkv = torch.randn((b * 577, 2304), generator=g).to(torch.bfloat16).cuda()
    for per_head, q_rows in ((False, 577), (True, 577), (False, 1)):
        out = torch.empty((b, 12, 577, 577) if per_head else (b, 577, 577), dtype=torch.float32, device='cuda')
        ms = timed(lambda: ops.attn_self_maps(qkv, b, 577, q_rows, per_head=per_head, out=out))
        print('B=%d: vitcap_attn_self_maps %s q_rows=%d %.3f ms per launch' % (b, 'per head' if per_head else 'head mean', q_rows, ms))
    A = torch.softmax(torch.randn((b, 577, 577), generator=g), -1).cuda()
    for rows in (1, 20):
        v = torch.rand((b, rows, 577), generator=g).cuda()
        out = torch.empty_like(v)
        print('n_img=%d rows=%d: vitcap_rollout_step %.3f ms per launch' % (b, rows, timed(lambda: ops.rollout_step(v, A, 0.5, out=out))))
