#!/usr/bin/env python
"""Match calibration on synthetic weights and synthetic images (xfr_amd/calibration.py): three lines, each the median of
--repeat runs that end in a device synchronise, after one untimed run.

  1. the embedding pass of the device path (calibration._device_encodings): device-resident ResNet-101 inputs encoded per batch_size chunk into
     one matrix, in images/s;
  2. the template and distance stage of mate_nonmate_dists for 1000 batches of 2 + 64 embeddings of 512 values: the two index tables built and
     uploaded, xfr_embed_templates (66 000 rows normalised), xfr_pair_dists (129 000 pairs), the distances back on the host, in ms; next to it the
     reference's numpy arithmetic (net_mate_nonmate_dists.py:123-128 per batch) on the same embeddings;
  3. xfr_nearest_rows at 9131 x 512, k = 8, excluding the self distance (eccv20.py:57-59 at VGGFace2's size), in ms, next to
     scipy.spatial.distance.pdist + squareform + argsort of every row on the same box's CPUs, and how many of the 9131 x 8 indices agree.

    python tools/calibration_probe.py [--images 5120] [--batch 128] [--repeat 5]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, repeat, sync):
    fn()
    sync()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return sorted(times)[len(times) // 2], out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--images', type=int, default=5120)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--batches', type=int, default=1000, help='batches of 2 + 64 of the distance stage')
    ap.add_argument('--subjects', type=int, default=9131)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--no-host', action='store_true', help='skip the numpy / scipy comparisons')
    args = ap.parse_args()
    import numpy as np
    import torch
    from xfr_amd import calibration as K
    from xfr_amd import synth
    from xfr_amd.models import resnet, whitebox as WB

    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    sync = torch.cuda.synchronize
    bb = resnet.ResNet([3, 4, 23, 3], num_classes=2)
    bb.load_state_dict(synth.synth_state_dict(bb, seed=0))
    bb.to(dev)
    wbn = WB.WhiteboxSTResnet(bb)
    wbn.default_max_batch = args.batch
    wb = WB.Whitebox(wbn)
    wb.batch_size = args.batch

    # 1. the embedding pass
    pool = synth.synth_smooth_images(args.batch, (3, 224, 224), seed=7, mean=resnet.MEAN_RGB).to(dev)
    images = [pool[i % args.batch] for i in range(args.images)]
    ms, (eng, enc) = median_ms(lambda: K._device_encodings(wb, images), args.repeat, sync)
    print('embedding pass: %d images of 3 x 224 x 224 (ResNet-101, synthetic) in chunks of %d: %.1f ms, %.0f images/s'
          % (args.images, args.batch, ms, args.images / ms * 1e3), flush=True)

    # 2. templates and distances of 1000 batches of 2 + 64
    m, D = K.NUM_NONMATES, 512
    n = args.batches * (2 + m)
    emb = torch.from_numpy(np.random.RandomState(0).randn(n, D).astype(np.float32)).to(dev)

    def stage():
        unit = eng.embed_templates(emb, np.arange(n), np.arange(n + 1), normalize_rows=True)
        base = np.arange(args.batches)[:, None] * (2 + m)
        mates = np.stack([base[:, 0], base[:, 0] + 1], axis=1)
        first = np.repeat(base + np.arange(2)[None, :], m, axis=1)
        second = np.tile(base + 2 + np.arange(m)[None, :], (1, 2))
        pairs = np.concatenate([mates, np.stack([first.ravel(), second.ravel()], axis=1)])
        return eng.pair_dists(unit, unit, pairs).cpu().numpy()
    ms, d = median_ms(stage, args.repeat, sync)
    line = 'template and distance stage: %d batches of 2 + %d (D = %d): %.2f ms on the device' % (args.batches, m, D, ms)
    if not args.no_host:
        emb_h = emb.cpu().numpy()

        def host():
            out = []
            for b in range(args.batches):
                e = emb_h[b * (2 + m):(b + 1) * (2 + m)]
                out.append(K._host_dists(e / np.linalg.norm(e, axis=1, keepdims=True)))
            return out
        hms, h = median_ms(host, min(args.repeat, 3), lambda: None)
        worst = max(np.abs(h[b][1].ravel() - d[args.batches + b * 2 * m:args.batches + (b + 1) * 2 * m]).max() for b in range(args.batches))
        line += ', %.1f ms in numpy on the host after the copy (largest difference %.1e)' % (hms, worst)
    print(line, flush=True)

    # 3. nearest rows at VGGFace2's size
    X = np.random.RandomState(1).randn(args.subjects, D).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Xd = torch.from_numpy(X).to(dev)
    ms, (idx, dist) = median_ms(lambda: eng.nearest_rows(Xd, Xd, 8, exclude_same_index=True), args.repeat, sync)
    line = 'nearest_rows: %d x %d, k = 8, self excluded: %.2f ms on the device' % (args.subjects, D, ms)
    if not args.no_host:
        from scipy.spatial.distance import pdist, squareform
        t0 = time.perf_counter()
        want = np.stack([np.argsort(row)[1:][0:8] for row in squareform(pdist(X, metric='euclidean'))])
        hms = (time.perf_counter() - t0) * 1e3
        line += ', %.0f ms for scipy pdist + squareform + argsort on the host (one run), %d of %d indices agree' % (
            hms, int((idx.cpu().numpy() == want).sum()), want.size)
    print(line, flush=True)


if __name__ == '__main__':
    main()
