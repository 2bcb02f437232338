#!/usr/bin/env python
"""One full STRise blackbox saliency map (xfr_amd.models.blackbox.STRise; python/xfr/models/blackbox.py:450-479) at the reference's scale:
ResNet-101, 6500 sparse masks, 50 gallery images, one reference, synthetic weights and images.  Prints one JSON line:

* sweep_masks_per_s   xfr_strise_score alone: masked probes, forward, scores -- everything between the masks and the score vector;
* forward_only_images_per_s   the ceiling of this workload: Whitebox.encode on batches that are already resident (the loop of
  tools/embeddings_sweep.py without its mask generation), measured in the same process, alternating with the sweep;
* sweep_vs_forward_only   images through the sweep (the probe and the padding included) per second over that ceiling: mask generation and scoring
  hide behind the forward when this is close to 1;
* merge_ms   compute_saliency_map: the selection on the host, the copy of the weights, xfr_strise_combine with its one stream synchronisation
  (median, like the sweep);  end_to_end_ms   evaluate(): prior, draws, fill, gallery encodes, sweep, merge.

    python tools/strise_probe.py --masks 6500 --batch 128 --gallery 50
"""
import argparse
import io
import json
import os
import sys
import time
from contextlib import redirect_stdout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--masks', type=int, default=6500)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--gallery', type=int, default=50)
    ap.add_argument('--elements', type=int, default=1)
    ap.add_argument('--rounds', type=int, default=3, help='alternating (forward-only, sweep) pairs; medians are reported')
    args = ap.parse_args()
    import numpy as np
    import torch
    from xfr_amd import synth
    from xfr_amd.models import blackbox as BB
    from xfr_amd.models import resnet, whitebox as WB

    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    bb = resnet.ResNet([3, 4, 23, 3], num_classes=2)
    bb.load_state_dict(synth.synth_state_dict(bb, seed=0))
    bb.to(dev)
    wbn = WB.WhiteboxSTResnet(bb)
    wbn.default_max_batch = args.batch
    wb = WB.Whitebox(wbn)
    wb.batch_size = args.batch
    base = synth.synth_smooth_images(3, (3, 224, 224), seed=1)                       # values in [0, 255]
    u8 = lambda t: t.permute(1, 2, 0).numpy().astype(np.uint8)                     # noqa: E731
    g = torch.Generator().manual_seed(3)
    gallery = [u8(torch.floor(0.8 * base[2] + 51.0 * torch.rand((3, 224, 224), generator=g))) for _ in range(args.gallery)]
    st = BB.STRise(probe=u8(base[0]), refs=[u8(base[1])], gallery=gallery, black_box='resnetv4_pytorch', num_masks=args.masks,
                   num_mask_elements=args.elements, net=wb)
    np.random.seed(0)

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()
    with redirect_stdout(io.StringIO()):
        st.evaluate()                                                                # warm-up: engine, streams, buffers, clocks
        t0 = sync()
        st.evaluate()
        end_to_end = sync() - t0
    eng, enc = st._engine()
    refs, gal = st._embed(st.refs), st._embed(st.gallery)
    probe, fill = torch.from_numpy(st.probe).to(dev), torch.from_numpy(st.fill_image).to(dev)
    cells, shifts, grid, scale = st._mask_args()
    n_batches = (args.masks + 1 + args.batch - 1) // args.batch
    resident = eng.strise_masked_probes(probe, fill, cells, shifts, grid, scale, 0, min(args.batch, args.masks))
    if resident.shape[0] < args.batch:
        resident = resident.repeat((args.batch + resident.shape[0] - 1) // resident.shape[0], 1, 1, 1)[:args.batch].contiguous()
    fwd, sweep = [], []
    for _ in range(max(1, args.rounds)):
        t0 = sync()
        for _ in range(n_batches):
            wb.encode(resident)
        fwd.append(sync() - t0)
        t0 = sync()
        scores, _ = eng.strise_score(probe, fill, cells, shifts, grid, scale, refs, gal, enc)
        sweep.append(sync() - t0)
    st.mask_scores = scores.cpu().numpy()
    merges = []
    for _ in range(max(1, args.rounds)):
        t0 = sync()
        st.compute_saliency_map()
        merges.append(sync() - t0)
    med = lambda v: sorted(v)[len(v) // 2]                                          # noqa: E731
    images = n_batches * args.batch
    out = {'workload': 'STRise map, ResNet-101 224x224, synthetic', 'masks': args.masks, 'batch': args.batch, 'gallery': args.gallery,
           'elements': args.elements, 'sweep_seconds': med(sweep), 'sweep_masks_per_s': args.masks / med(sweep),
           'sweep_images_per_s': images / med(sweep), 'forward_only_images_per_s': images / med(fwd),
           'sweep_vs_forward_only': med(fwd) / med(sweep), 'merge_ms': 1e3 * med(merges), 'end_to_end_ms': 1e3 * end_to_end,
           'sweeps_seconds': sweep, 'forward_only_seconds': fwd, 'merges_seconds': merges,
           'merge_includes': 'the selection on the host (np.percentile), the copy of the weights and the call\'s one stream synchronisation',
           'forward_only_is': 'Whitebox.encode on one resident batch, %d times: no mask generation at all' % n_batches, 'selected_masks': int(st.selected_indices.sum()),
           'map_finite': bool(np.isfinite(st.saliency_map).all()), 'reported': 'medians of %d alternating pairs in one process' % len(sweep)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
