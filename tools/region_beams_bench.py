"""Region captions under beam search: the kernel measurement of docs/LAB_region_beams.md.

  kernel B K iters      launch the beam decode-step attention `iters` times per case at B images x K beams, the cases one after the
                        other (for rocprofv3 --kernel-trace; the launches are told apart by their order).  Prints device-event times too.
  summary CSV iters     per-case kernel times from the kernel trace of such a run
"""
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S_VIS, T, L = 578, 10, 20
CASES = ('plain kernel', 'masked, all visible', 'masked, 6x6 centre + cls', 'masked, all hidden')


def case_masks():
    """bool (578,) per masked case, in the order of CASES[1:]."""
    import torch
    from vitcap_amd.regions import box_masks
    return [torch.ones(S_VIS, dtype=torch.bool), box_masks(torch.tensor([[9, 9, 15, 15]]))[0], torch.zeros(S_VIS, dtype=torch.bool)]


def live_blocks(mask):
    """(16-key blocks of phase 1a, 32-key blocks of phase 2a) a launch loads and multiplies under `mask` (None: all 37 / 19)."""
    if mask is None:
        return (S_VIS + 15) // 16, 19
    return (sum(bool(mask[k:k + 16].any()) for k in range(0, S_VIS, 16)), sum(bool(mask[k:k + 32].any()) for k in range(0, S_VIS, 32)))


def kernel(B, K, iters):
    import torch
    from vitcap_amd import ops
    from vitcap_amd._lib import lib
    from vitcap_amd.occlusion import pack_visible
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) * 2).to(torch.bfloat16).cuda()
    step, vis, cache = rnd(B * K * 2, 2304), rnd(B * S_VIS, 2304), rnd(B * K, L, 2, 768)
    vt = torch.empty((B, 12, 64, 608), device='cuda', dtype=torch.bfloat16)
    out = torch.empty((B * K * 2, 768), device='cuda', dtype=torch.bfloat16)
    p = lambda x: x.data_ptr()
    ops.check(lib.vitcap_attn_beam_vt(p(vis), p(vt), B, S_VIS, None), 'attn_beam_vt')
    masks = [pack_visible(m[None].expand(B, -1)).cuda().contiguous() for m in case_masks()]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, mask in zip(CASES, [None] + masks):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            if mask is None:
                rc = lib.vitcap_attn_decode_beams(p(step), p(vis), p(vt), p(cache), p(out), B, K, S_VIS, T, L, 0.125, None)
            else:
                rc = lib.vitcap_attn_decode_beam_groups_masked(p(step), p(vis), p(vt), p(cache), p(out), B, K, 1, S_VIS, T, L, 0.125,
                                                               p(mask), 19, None)
            ops.check(rc, name)
        e1.record()
        torch.cuda.synchronize()
        print('%-26s %7.2f us per launch back to back (device events)' % (name, e0.elapsed_time(e1) / iters * 1e3))


def summary(path, iters):
    rows = [r for r in csv.DictReader(open(path)) if 'attn_decode_beam_kernel' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    assert len(rows) == len(CASES) * iters, (len(rows), len(CASES), iters)
    masks = [None] + case_masks()
    for i, name in enumerate(CASES):
        chunk = rows[i * iters + iters // 5:(i + 1) * iters]            # the first fifth of a case warms up
        us = sorted((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in chunk)
        b16, b32 = live_blocks(masks[i])
        print('%-26s %4d launches  median %6.2f us  mean %6.2f us  min %6.2f us  %2d of 37 K blocks, %2d of 19 V^T blocks  (%s)'
              % (name, len(us), us[len(us) // 2], sum(us) / len(us), us[0], b16, b32, chunk[0]['Kernel_Name'][-40:]))


if __name__ == '__main__':
    if sys.argv[1] == 'kernel':
        kernel(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    else:
        summary(sys.argv[2], int(sys.argv[3]))
