"""Token-alternatives timing: ImageCaptioning.alternatives (k = 5, 16) at B images x K captions per image against score(one_pass=True)
on the same captions, and for one full 2048-row chunk of the vocabulary GEMM the alternatives kernel alone next to that chunk's GEMM
and vitcap_score_rows, as ms and as GB/s of the 250 MB one read of the chunk costs (run on the GPU box).
Usage: python tools/alternatives_bench.py [B=64] [K list=1,5] [iters=10]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vitcap_amd import ops
from vitcap_amd import weights as W
from vitcap_amd.model import ImageCaptioning

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
KS = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else '1,5').split(',')]
ITERS = int(sys.argv[3]) if len(sys.argv) > 3 else 10
V, VP, CHUNK = 30522, 30592, 2048


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
print('B=%d: generate %.2f ms per call' % (B, timed(lambda: m.generate(img))))
for K in KS:
    caps = ids[:, 0].repeat_interleave(K, 0).clone()
    for k in range(1, K):                       # the K captions of an image differ in one word each
        caps[k::K, 1 + k % 18] = 2000 + k
    print('B=%d K=%d: score one pass %.2f ms per call' % (B, K, timed(lambda: m.score(img, caps, seqs_per_image=K, one_pass=True))))
    for k in (5, 16):
        ms = timed(lambda: m.alternatives(img, caps, seqs_per_image=K, k=k))
        print('B=%d K=%d: alternatives k=%d %.2f ms per call' % (B, K, k, ms))

# one full chunk: 2048 probe rows of 108 captions (every row live), random logits of the vocabulary GEMM's own making
g = torch.Generator().manual_seed(0)
n_caps = -(-CHUNK // (L - 1))
caps = torch.randint(2000, 30000, (n_caps, L), generator=g)
caps[:, 0] = 101
capd = caps.cuda()
hid = torch.randn((CHUNK, 768), generator=g).to(torch.bfloat16).cuda()
dec_w = (torch.randn((VP, 768), generator=g) * 0.05).to(torch.bfloat16).cuda()
dec_b = torch.zeros(VP, dtype=torch.float32).cuda()
logits = torch.empty((CHUNK, VP), dtype=torch.float32, device='cuda')
mb = CHUNK * V * 4 / 1e6
ms = timed(lambda: ops.gemm_bias_act(hid, dec_w, dec_b, out=logits))
print('chunk %d x %d: vocabulary GEMM %.3f ms (writes %.0f MB: %.0f GB/s)' % (CHUNK, VP, ms, CHUNK * VP * 4 / 1e6, CHUNK * VP * 4 / 1e6 / ms))
# the row kernels through the C entry points with their arguments made once: the wrappers of vitcap_amd/ops.py cost more host time per
# call than these kernels run, and the stream would drain between launches
import ctypes as C
from vitcap_amd._lib import lib
ITERS = 10 * ITERS
P = lambda t: C.c_void_p(t.data_ptr())
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
st = ops.score_rows(logits, capd)
args = (P(logits), VP, V, P(capd), None, 0, CHUNK, n_caps, L, 102, None, 0, P(st['sum_lp']), P(st['cnt']), P(st['token_logprobs']),
        P(st['ids']), P(st['last_tok']), P(st['logprob']), stream)
ms = timed(lambda: lib.vitcap_score_rows(*args))
print('chunk: vitcap_score_rows %.3f ms (one read of the chunk is %.0f MB: %.0f GB/s if read once; the kernel reads each row twice)'
      % (ms, mb, mb / ms))
for k in (1, 5, 16):
    out = ops.score_rows_alts(logits, capd, k)
    args = (P(logits), VP, V, P(capd), None, 0, CHUNK, n_caps, L, 102, None, 0, k, P(out['ids']), P(out['logprobs']), P(out['rank']),
            P(out['entropy']), stream)
    ms = timed(lambda: lib.vitcap_score_rows_alts(*args))
    print('chunk: vitcap_score_rows_alts k=%d %.3f ms (%.0f MB read once: %.0f GB/s)' % (k, ms, mb, mb / ms))
