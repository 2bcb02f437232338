#!/usr/bin/env python
"""The grouped 3x3 layers of ResNeXt-50 32x4d on the grouped-convolution kernel (xfr_amd/csrc/conv_group.hip, configuration 13), shape by shape.

For each grouped layer shape of ResNeXt-50 32x4d at batch 32 (C -> C channels in 32 groups, the four stride-1 shapes and the three stage-opening
stride-2 ones): the dual forward launch (W and relu(W) from one staged input), the backward-data launch of one gradient stream (stride 1) or the
four phase launches (stride 2), each with

  * the time per launch: HIP events around the launch (the engine's per-launch profile, xfr_engine_set_profile), median of --rounds sweeps;
  * useful TFLOP/s: 2 K M Cout [x 2 for the dual launch] with the K of one group, over that time;
  * the algorithmic bytes (X once, Y once [twice for the dual launch], W once; an accumulating launch reads Y as well), the rate they were moved at,
    and the launch time over the time those bytes take at 6.3 TB/s, the chip's measured HBM rate: how far the launch is from its HBM time.

Then maps/s of resnext50_32x4d through Whitebox.contrastive_triplet_ebp_batch at batch 32, next to tv_resnet.resnet50 in the same process (host
clock around calls that end in a device synchronise).  Everything is reported; nothing is gated.

    python tools/grouped_probe.py [--rounds 7] [--out profiles/r19/grouped_probe.txt]
"""
import argparse
import csv
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (channels, per-group channels, input H, stride) of the grouped 3x3 layers of ResNeXt-50 32x4d at 224 x 224, and how many layers have the shape
SHAPES = ((128, 4, 56, 1, 3), (256, 8, 56, 2, 1), (256, 8, 28, 1, 3), (512, 16, 28, 2, 1), (512, 16, 14, 1, 5), (1024, 32, 14, 2, 1), (1024, 32, 7, 1, 2))
GROUPS = 32
BATCH = 32
HBM = 6.3e12
CFG_GROUP = 13


def _program(c, h, stride):
    """conv 1x1 C -> C, ReLU, grouped conv 3x3 C -> C with the given stride, ReLU, global average pool, Linear."""
    from xfr_amd.program import Program
    p = Program((c, h, h))
    t = p.relu_(p.conv(0, 'conv0', c, 1, bias=False))
    t = p.relu_(p.conv(t, 'conv1', c, 3, stride=stride, pad=1, bias=False, groups=GROUPS))
    ho = (h + 2 - 3) // stride + 1
    t = p.avgpool(t, ho, 1)
    return p, p.mark('classify', p.linear(t, 'fc', 8, (1, 1), bias=False))


def _weights(c, ci):
    import torch
    g = torch.Generator().manual_seed(c)
    return {'conv0.weight': torch.randn((c, c, 1, 1), generator=g) / c ** 0.5, 'conv1.weight': torch.randn((c, ci, 3, 3), generator=g) / (9 * ci) ** 0.5,
            'fc.weight': torch.randn((8, c), generator=g) / c ** 0.5}


def _launches(eng, x, st, seed, path):
    """The grouped launches of one profiled sweep -> list of dicts (kind, nhalves, K, M, accumulate, ms)."""
    import torch
    if os.path.exists(path):
        os.remove(path)
    eng.profile_csv(path)
    eng.ebp(x, st, seed)
    torch.cuda.synchronize()
    eng.profile_csv(None)
    out = []
    with open(path) as f:
        # columns: Cout, nhalves, K, M, kh, stride, out_stride, relu_in, accumulate, ms, TFLOP/s, cfg
        for r in csv.reader(f):
            if not r or int(r[11]) != CFG_GROUP:
                continue
            kind = 'phase' if int(r[6]) > 1 else ('forward' if not out else 'backward')
            out.append(dict(kind=kind, nhalves=int(r[1]), K=int(r[2]), M=int(r[3]), acc=int(r[8]), ms=float(r[9])))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r19', 'grouped_probe.txt'))
    ap.add_argument('--no-net', action='store_true', help='skip the whole-network throughput')
    args = ap.parse_args()
    import torch
    from xfr_amd.engine import Engine
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    tmp = tempfile.mkdtemp()
    med = lambda t: sorted(t)[len(t) // 2]      # noqa: E731
    lines = ['grouped_probe: the grouped 3x3 layers of ResNeXt-50 32x4d at batch %d on configuration %d (fp32 MFMA 16x16x4, row blocks of 16 channels of one group); '
             'one gradient stream; medians of %d sweeps' % (BATCH, CFG_GROUP, args.rounds),
             'time: HIP events around each launch (xfr_engine_set_profile).  useful TFLOP/s: 2 K M Cout (x 2 dual) with the K of one group.  bytes: X once, Y once per '
             'half (and read once where the launch accumulates), W once.  x HBM: launch time over bytes / 6.3 TB/s (the measured HBM rate)',
             'everything is reported, nothing gated.']
    for c, ci, h, stride, count in SHAPES:
        prog, st = _program(c, h, stride)
        eng = Engine(prog, BATCH, dev)
        eng.load_weights(_weights(c, ci))
        eng.set_mode('norelu')
        g = torch.Generator().manual_seed(h)
        x = torch.randn((BATCH, c, h, h), generator=g).to(dev)
        seed = torch.rand((1, BATCH, 8), generator=g).to(dev)
        eng.ebp(x, st, seed)          # untimed: allocations, first launches
        eng.set_profile(True)
        runs = [_launches(eng, x, st, seed, os.path.join(tmp, 'p.csv')) for _ in range(args.rounds)]
        eng.close()
        n = len(runs[0])
        assert n == (2 if stride == 1 else 5) and all(len(r) == n for r in runs), runs[0]
        ho = (h + 2 - 3) // stride + 1
        lines.append('%4d -> %4d in %d groups (Ci = Co = %d), %2d^2 -> %2d^2, stride %d, %d layer%s of the net:' % (c, c, GROUPS, ci, h, ho, stride, count, '' if count == 1 else 's'))
        tot = 0.0
        for i in range(n):
            L = runs[0][i]
            ms = med([r[i]['ms'] for r in runs])
            flops = 2.0 * L['K'] * L['M'] * c * L['nhalves']
            hw_in = h * h if L['kind'] == 'forward' else ho * ho
            y = c * L['M'] * 4.0 * L['nhalves'] * (2 if L['acc'] else 1)
            bytes_ = c * BATCH * hw_in * 4.0 + y + c * L['K'] * 4.0 * L['nhalves']
            t_hbm = bytes_ / HBM * 1e3
            tot += ms if L['kind'] != 'forward' else 0.0
            lines.append('    %-8s K %3d M %6d  %.4f ms (sweeps %.4f .. %.4f)  %6.2f useful TFLOP/s  %6.1f MB algorithmic, %5.2f TB/s  %5.2f x HBM time'
                         % (L['kind'] + (' dual' if L['nhalves'] == 2 else ''), L['K'], L['M'], ms, min(r[i]['ms'] for r in runs), max(r[i]['ms'] for r in runs),
                            flops / (ms * 1e-3) / 1e12, bytes_ / 1e6, bytes_ / (ms * 1e-3) / 1e12, ms / t_hbm))
        if stride == 2:
            lines.append('    phases summed: %.4f ms' % tot)
    if not args.no_net:
        from xfr_amd.models import tv_resnet, whitebox as WB
        for name in ('resnext50_32x4d', 'resnet50'):
            bb = getattr(tv_resnet, name)(num_classes=16).to(dev)
            wbn = WB.WhiteboxTVResnet(bb)
            wb = WB.Whitebox(wbn)
            g = torch.Generator().manual_seed(5)
            x = torch.randn((BATCH, 3, 224, 224), generator=g).to(dev)
            xm = torch.randn((BATCH, 2048), generator=g).to(dev) / 2500
            xn = torch.randn((BATCH, 2048), generator=g).to(dev) / 2500
            wb.contrastive_triplet_ebp_batch(x, xm, xn)
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                out = wb.contrastive_triplet_ebp_batch(x, xm, xn)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            assert bool(torch.isfinite(torch.as_tensor(out)).all())
            lines.append('tv_resnet.%s, 224 x 224, contrastive_triplet_ebp_batch at batch %d (seeded random weights and images; host clock around synchronised calls): '
                         '%.1f ms per call (rounds %.1f .. %.1f), %.1f maps/s' % (name, BATCH, med(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3, BATCH / med(ts)))
            wbn.engine().close()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
