"""Region captions: the measurements of docs/LAB_regions.md.

  kernel B iters        launch the decode-step attention `iters` times per case, the cases one after the other (for
                        rocprofv3 --kernel-trace; the launches are told apart by their order).  Prints device-event times too.
  summary CSV B iters   per-case kernel times from the kernel trace of such a run, with bytes moved and TB/s
  regions B             caption_regions (2 x 2 tiling, one pass of 4 sequences per image) against four single-region decodes and
                        four unmasked decodes on the same encoded batch, ms per call
"""
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S_VIS, T, L = 578, 10, 20
CASES = ('plain kernel', 'masked, all visible', 'masked, 6x6 top-left + cls', 'masked, 6x6 centre + cls', 'masked, 8x24 band + cls',
         'masked, all hidden')


def case_masks():
    """bool (578,) per masked case, in the order of CASES[1:]."""
    import torch
    from vitcap_amd.regions import box_masks
    boxes = torch.tensor([[0, 0, 6, 6], [9, 9, 15, 15], [8, 0, 16, 24]])
    m = box_masks(boxes)
    return [torch.ones(S_VIS, dtype=torch.bool), m[0], m[1], m[2], torch.zeros(S_VIS, dtype=torch.bool)]


def bytes_moved(mask, B, skip=True):
    """Bytes one launch reads at least: K and V head slices of every visual key it loads (all 12 heads: whole rows' K|V thirds), the
    text rows and the step rows.  With the sweep skip a whole 128-key sweep is loaded iff one of its keys is visible; the last 66
    visual keys share the mixed sweep, which is always loaded."""
    full = S_VIS & ~127
    keys = S_VIS - full
    for k0 in range(0, full, 128):
        if mask is None or not skip or bool(mask[k0:k0 + 128].any()):
            keys += 128
    per_seq = keys * 2 * 768 * 2 + (T - 1) * 2 * 768 * 2 + 2 * 2304 * 2 + 2 * 768 * 2
    return B * per_seq


def kernel(B, iters):
    import torch
    from vitcap_amd import ops
    from vitcap_amd.occlusion import pack_visible
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) * 2).to(torch.bfloat16).cuda()
    step, vis, cache = rnd(B * 2, 2304), rnd(B * S_VIS, 2304), rnd(B, L, 2, 768)
    masks = [pack_visible(m[None].expand(B, -1)).cuda().contiguous() for m in case_masks()]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, mask in zip(CASES, [None] + masks):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            if mask is None:
                ops.attn_decode_step(step, vis, cache, B, S_VIS, T, max_len=L)
            else:
                ops.attn_decode_step_masked(step, vis, cache, mask, B, S_VIS, T, max_len=L)
        e1.record()
        torch.cuda.synchronize()
        print('%-28s %7.2f us per launch back to back (device events)' % (name, e0.elapsed_time(e1) / iters * 1e3))


def summary(path, B, iters, skip):
    rows = [r for r in csv.DictReader(open(path)) if 'attn_decode_kernel' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    assert len(rows) == len(CASES) * iters, (len(rows), len(CASES), iters)
    masks = [None] + case_masks()
    for i, name in enumerate(CASES):
        chunk = rows[i * iters + iters // 5:(i + 1) * iters]            # the first fifth of a case warms up
        us = sorted((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in chunk)
        med, mean = us[len(us) // 2], sum(us) / len(us)
        nbytes = bytes_moved(masks[i], B, skip)
        print('%-28s %4d launches  median %6.2f us  mean %6.2f us  %6.1f MB  %5.2f TB/s  (%s)'
              % (name, len(us), med, mean, nbytes / 1e6, nbytes / med / 1e6, chunk[0]['Kernel_Name'][:48]))


def regions(B):
    import torch
    from vitcap_amd import weights as W
    from vitcap_amd.model import ImageCaptioning
    from vitcap_amd.occlusion import pack_visible
    from vitcap_amd.regions import box_masks, grid_regions
    m = ImageCaptioning(tie_weights=True, tagemb='cls').load_recipe(0).eval()
    m.pack('cuda')
    img = torch.from_numpy(W.gen_image_batch(B, 77)).cuda().to(torch.bfloat16)
    boxes = grid_regions(2)
    masks = box_masks(boxes)
    o = m.gen_options(num_beams=1, do_sample=False, num_return_sequences=1, num_keep_best=1, use_graph=False)
    words = [pack_visible(masks[r:r + 1].expand(B, -1)) for r in range(4)]
    ones = pack_visible(torch.ones(B, S_VIS, dtype=torch.bool))

    def timed(fn, n=5):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    m.caption_regions(img, boxes)                                       # encodes; everything below decodes on this prefill
    t_regions = timed(lambda: m.caption_regions_encoded(boxes))
    t_single = timed(lambda: [m.run(None, o, vis=w) for w in words])
    t_full = timed(lambda: [m.run(None, o, vis=ones) for _ in range(4)])
    t_whole = timed(lambda: m.caption_regions(img, boxes))
    print('B=%d, 2 x 2 tiling, greedy, max_length 20, decode on the encoded batch:' % B)
    print('  caption_regions_encoded (one pass, 4 sequences per image)  %7.2f ms' % t_regions)
    print('  four single-region masked decodes (1 sequence per image)   %7.2f ms' % t_single)
    print('  four all-visible masked decodes (1 sequence per image)     %7.2f ms' % t_full)
    print('  caption_regions with the encoder pass                      %7.2f ms' % t_whole)


if __name__ == '__main__':
    mode = sys.argv[1]
    if mode == 'kernel':
        kernel(int(sys.argv[2]), int(sys.argv[3]))
    elif mode == 'summary':
        summary(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), skip=(sys.argv[5:] or ['skip'])[0] == 'skip')
    else:
        regions(int(sys.argv[2]))
