#!/usr/bin/env python
"""The inpainting game of one probe at the paper's scale (xfr_amd.inpainting_score.score_maps; python/xfr/inpainting_game/inpainting_game.py:80-146):
ResNet-101, 8 saliency maps x 101 percent-density levels per call, synthetic weights, images and maps.  Prints one JSON line:

* games_per_s         maps scored per second by xfr_inpaint_score: masks, hybrids, forward, distances (a game is one map at 101 levels);
* mask_stage_ms       the order statistics alone (xfr_inpaint_debug_masks on the same 8 maps): sort, running sum, first_on;
* sweep_images_per_s  hybrids through the call per second, the padding of the last batch included;
* forward_only_images_per_s   the ceiling: Whitebox.encode on one resident batch, as many times (what tools/embeddings_sweep.py measures), in the
  same process, alternating with the sweep;
* sweep_vs_forward_only       the share of that ceiling the sweep reaches.

    python tools/inpainting_score_probe.py --maps 8 --batch 128 > profiles/r9/inpainting_score_probe.txt

--method percent-pixels: the levels are np.percentile thresholds of every map, computed on the host once before the timed rounds
(host_thresholds_ms), and travel as explicit thresholds with the maps' totals (xfr_inpaint_score_ex).
--blur PCT: soft-edged masks of sigma PCT per cent of 224 pixels.  The rounds then alternate the hard-mask sweep, the blurred sweep and the forward
alone in one process, and the line adds blur_sweep_images_per_s and blur_vs_hard_sweep, the share of the hard-mask rate the blurred sweep reaches:

    python tools/inpainting_score_probe.py --blur 4 > profiles/r10/inpainting_soft_probe.txt
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--maps', type=int, default=8)
    ap.add_argument('--levels', type=int, default=101)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=5, help='alternating (forward-only, sweep, masks) triples; medians are reported')
    ap.add_argument('--blur', type=float, default=None, metavar='PCT', help='mask_blur_sigma: also time the sweep with soft-edged masks')
    ap.add_argument('--method', choices=('percent-density', 'percent-pixels'), default='percent-density')
    args = ap.parse_args()
    import numpy as np
    import torch
    from xfr_amd import inpainting_score as S
    from xfr_amd import synth
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
    base = synth.synth_smooth_images(2, (3, 224, 224), seed=1, mean=resnet.MEAN_RGB)
    orig = base[0].to(dev)
    twin = orig.clone()
    twin[:, 60:160, 50:150] = base[1][:, 60:160, 50:150].to(dev)
    rng = np.random.RandomState(0)
    yy, xx = np.mgrid[0:224, 0:224].astype(np.float64)
    maps = np.stack([np.maximum(sum(rng.rand() * np.exp(-((yy - rng.uniform(40, 180)) ** 2 + (xx - rng.uniform(40, 180)) ** 2) / (2 * rng.uniform(15, 45) ** 2))
                                    for _ in range(5)) - 0.1, 0.0) for _ in range(args.maps)])
    maps_d = torch.from_numpy(maps).to(dev)
    noise = torch.from_numpy(np.random.RandomState(1).rand(224, 224)).to(dev)
    levels = np.linspace(0, 100, args.levels)
    eng = wb._engine(args.batch)
    enc = wb.net._mark('encode')
    gal = wb.encode(torch.stack([orig, twin]))
    gal = gal / gal.norm(dim=1, keepdim=True)
    kw, host_ms = dict(noise=noise), None
    if args.method == 'percent-pixels':
        t0 = time.perf_counter()
        levels, totals = S._pixel_thresholds(maps, levels, noise.cpu().numpy(), 1e-9, True)
        host_ms = 1e3 * (time.perf_counter() - t0)
        kw.update(method='thresholds', totals=totals, levels_per_map=True)
    blur_kw = None
    if args.blur:
        blur_kw = dict(kw, blur_kernel=S.gaussian_kernel1d(args.blur * 224 / 100.0), blur_levels=np.linspace(0, 100, args.levels) != 100)
    total = args.maps * args.levels
    n_batches = (total + args.batch - 1) // args.batch
    resident = eng.inpaint_blends(maps_d, levels, orig, twin, first=0, count=min(args.batch, total), **kw)
    if resident.shape[0] < args.batch:
        resident = resident.repeat((args.batch + resident.shape[0] - 1) // resident.shape[0], 1, 1, 1)[:args.batch].contiguous()

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()
    cls, _, _ = eng.inpaint_score(maps_d, levels, orig, twin, gal[0], gal[1], enc, **kw)      # warm-up: streams, buffers, clocks
    fwd, sweep, masks, soft = [], [], [], []
    for _ in range(max(1, args.rounds)):
        t0 = sync()
        for _ in range(n_batches):
            wb.encode(resident)
        fwd.append(sync() - t0)
        t0 = sync()
        cls, pg, pr = eng.inpaint_score(maps_d, levels, orig, twin, gal[0], gal[1], enc, **kw)
        sweep.append(sync() - t0)
        if blur_kw:
            t0 = sync()
            cls_b, pg_b, pr_b = eng.inpaint_score(maps_d, levels, orig, twin, gal[0], gal[1], enc, **blur_kw)
            soft.append(sync() - t0)
        t0 = sync()
        eng.inpaint_masks(maps_d, levels, **kw)
        masks.append(sync() - t0)
    med = lambda v: sorted(v)[len(v) // 2]                                          # noqa: E731
    images = n_batches * args.batch
    cls = cls.cpu().numpy()
    out = {'workload': 'inpainting game, ResNet-101 224x224, synthetic', 'method': args.method, 'maps': args.maps, 'levels': args.levels, 'batch': args.batch,
           'sweep_seconds': med(sweep), 'games_per_s': args.maps / med(sweep), 'mask_stage_ms': 1e3 * med(masks),
           'mask_stage_ms_per_map': 1e3 * med(masks) / args.maps, 'sweep_images_per_s': images / med(sweep),
           'forward_only_images_per_s': images / med(fwd), 'sweep_vs_forward_only': med(fwd) / med(sweep), 'hybrids': total, 'padding': images - total,
           'sweeps_seconds': sweep, 'forward_only_seconds': fwd, 'mask_stage_seconds': masks,
           'forward_only_is': 'Whitebox.encode on one resident batch, %d times: no masks, no blends, no distances' % n_batches,
           'first_level_as_twin': [int(np.argmax(c)) if c.any() else -1 for c in cls], 'finite': bool(torch.isfinite(pg).all() and torch.isfinite(pr).all()),
           'reported': 'medians of %d alternating triples in one process' % len(sweep)}
    if host_ms is not None:
        out['host_thresholds_ms'] = host_ms
    if blur_kw:
        out.update({'blur_sigma_percent': args.blur, 'blur_radius': len(blur_kw['blur_kernel']) // 2, 'blur_sweep_seconds': med(soft),
                    'blur_sweep_images_per_s': images / med(soft), 'blur_vs_hard_sweep': med(sweep) / med(soft), 'blur_sweeps_seconds': soft,
                    'blur_first_level_as_twin': [int(np.argmax(c)) if c.any() else -1 for c in cls_b.cpu().numpy()],
                    'blur_finite': bool(torch.isfinite(pg_b).all() and torch.isfinite(pr_b).all())})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
