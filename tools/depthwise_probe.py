#!/usr/bin/env python
"""The depthwise layers of MobileNetV1 on the vector-ALU depthwise kernel (xfr_amd/csrc/conv_depthwise.hip, configuration 14) and on the grouped MFMA
kernel they ran on before (conv_group.hip, configuration 13; fusion-mask bit 10 keeps them there), shape by shape.

For each depthwise shape of MobileNetV1 at 224 x 224 and batch 32 (C channels in C groups, 3x3, stride 1 and 2, and the 7x7 global depthwise head):
the dual forward launch (W and relu(W) from one staged input), the backward-data launch of one gradient stream (stride 1) or the four phase launches
(stride 2), each with

  * the time per launch on either configuration: HIP events around the launch (the engine's per-launch profile, xfr_engine_set_profile), the same
    process and engine, the settings alternating 13, 14, 13 in every round, medians of --rounds rounds;
  * the spread between the medians of the two configuration-13 sweeps: the yardstick a difference has to exceed to count;
  * the algorithmic bytes (X once, Y once per half, and one read of Y where the launch accumulates) and the launch time over the time those bytes
    take at 6.3 TB/s, the chip's measured HBM rate.

Then maps/s of mobilenet_v1 through Whitebox.contrastive_triplet_ebp_batch at batch 32 with bit 10 off and on, alternating, three runs each (host
clock around calls that end in a device synchronise).  Everything is reported.  The one decision taken from the table: a shape class on which
configuration 14 is not faster than 13 by more than the spread does not go to the new kernel (launch_conv_depthwise).

    python tools/depthwise_probe.py [--rounds 7] [--out profiles/r20/depthwise_probe.txt]
"""
import argparse
import csv
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (channels, input H, kernel, stride, pad) of the depthwise layers of MobileNetV1 at 224 x 224, and the global depthwise head
SHAPES = ((32, 112, 3, 1, 1), (64, 112, 3, 2, 1), (128, 56, 3, 1, 1), (128, 56, 3, 2, 1), (256, 28, 3, 1, 1), (256, 28, 3, 2, 1),
          (512, 14, 3, 1, 1), (512, 14, 3, 2, 1), (1024, 7, 3, 1, 1), (1024, 7, 7, 1, 0))
BATCH = 32
HBM = 6.3e12
CFGS = (13, 14)
KEEP_ON_13 = 1 << 10


def _program(c, h, k, stride, pad):
    """conv 1x1 C -> C, ReLU, depthwise conv k x k with the given stride, ReLU, global average pool, Linear."""
    from xfr_amd.program import Program
    p = Program((c, h, h))
    t = p.relu_(p.conv(0, 'conv0', c, 1, bias=False))
    t = p.relu_(p.conv(t, 'conv1', c, k, stride=stride, pad=pad, bias=False, groups=c))
    ho = (h + 2 * pad - k) // stride + 1
    if ho > 1:
        t = p.avgpool(t, ho, 1)
    return p, p.mark('classify', p.linear(t, 'fc', 8, (1, 1), bias=False)), ho


def _weights(c, k):
    import torch
    g = torch.Generator().manual_seed(c + k)
    return {'conv0.weight': torch.randn((c, c, 1, 1), generator=g) / c ** 0.5, 'conv1.weight': torch.randn((c, 1, k, k), generator=g) / k,
            'fc.weight': torch.randn((8, c), generator=g) / c ** 0.5}


def _launches(eng, x, st, seed, path, cfg):
    """The grouped launches of one profiled sweep, which must all have run on `cfg` -> list of dicts (kind, nhalves, K, M, accumulate, ms)."""
    import torch
    if os.path.exists(path):
        os.remove(path)
    eng.set_epilogue_fusion(3 | (KEEP_ON_13 if cfg == 13 else 0))
    eng.profile_csv(path)
    eng.ebp(x, st, seed)
    torch.cuda.synchronize()
    eng.profile_csv(None)
    out = []
    with open(path) as f:
        # columns: Cout, nhalves, K, M, kh, stride, out_stride, relu_in, accumulate, ms, TFLOP/s, cfg
        for r in csv.reader(f):
            if not r or int(r[11]) not in CFGS:
                continue
            assert int(r[11]) == cfg, (cfg, r)
            kind = 'phase' if int(r[6]) > 1 else ('forward' if not out else 'backward')
            out.append(dict(kind=kind, nhalves=int(r[1]), K=int(r[2]), M=int(r[3]), acc=int(r[8]), ms=float(r[9])))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r20', 'depthwise_probe.txt'))
    ap.add_argument('--no-net', action='store_true', help='skip the whole-network throughput')
    args = ap.parse_args()
    import torch
    from xfr_amd.engine import Engine
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    tmp = tempfile.mkdtemp()
    med = lambda t: sorted(t)[len(t) // 2]      # noqa: E731
    lines = ['depthwise_probe: the depthwise layers of MobileNetV1 at batch %d on configuration 14 (fp32 on the vector ALU, one LDS staging) and on configuration 13 '
             '(fp32 MFMA 16x16x4, one live row of 16; fusion-mask bit 10); one gradient stream; every round runs 13, 14, 13; medians of %d rounds' % (BATCH, args.rounds),
             'time: HIP events around each launch (xfr_engine_set_profile).  spread: |median of the first - median of the second configuration-13 sweep|.  bytes: X once, '
             'Y once per half (and read once where the launch accumulates).  x HBM: launch time on 14 over bytes / 6.3 TB/s (the measured HBM rate)',
             'verdict: 14 where its median is below the lower configuration-13 median by more than the spread, else 13.  everything is reported.']
    for c, h, k, stride, pad in SHAPES:
        prog, st, ho = _program(c, h, k, stride, pad)
        eng = Engine(prog, BATCH, dev)
        eng.load_weights(_weights(c, k))
        eng.set_mode('norelu')
        g = torch.Generator().manual_seed(h)
        x = torch.randn((BATCH, c, h, h), generator=g).to(dev)
        seed = torch.rand((1, BATCH, 8), generator=g).to(dev)
        for cfg in CFGS:                  # untimed: allocations, first launches
            eng.set_epilogue_fusion(3 | (KEEP_ON_13 if cfg == 13 else 0))
            eng.ebp(x, st, seed)
        eng.set_profile(True)
        path = os.path.join(tmp, 'p.csv')
        a1, b, a2 = [], [], []
        for _ in range(args.rounds):
            a1.append(_launches(eng, x, st, seed, path, 13))
            b.append(_launches(eng, x, st, seed, path, 14))
            a2.append(_launches(eng, x, st, seed, path, 13))
        eng.close()
        n = len(b[0])
        assert n == (2 if stride == 1 else 5) and all(len(r) == n for r in a1 + b + a2), b[0]
        lines.append('%4d channels, %dx%d, %3d^2 -> %3d^2, stride %d, pad %d:' % (c, k, k, h, ho, stride, pad))
        tot = {13: 0.0, 14: 0.0}
        for i in range(n):
            L = b[0][i]
            m1, m14, m2 = med([r[i]['ms'] for r in a1]), med([r[i]['ms'] for r in b]), med([r[i]['ms'] for r in a2])
            spread = abs(m1 - m2)
            m13 = min(m1, m2)
            hw_in = h * h if L['kind'] == 'forward' else ho * ho
            bytes_ = c * BATCH * hw_in * 4.0 + c * L['M'] * 4.0 * L['nhalves'] * (2 if L['acc'] else 1)
            t_hbm = bytes_ / HBM * 1e3
            if L['kind'] != 'forward':
                tot[13] += m13
                tot[14] += m14
            lines.append('    %-13s K %3d M %6d  cfg 14 %.4f ms (%.4f .. %.4f)  cfg 13 %.4f / %.4f ms, spread %.4f  13 / 14 = %5.2f  %6.1f MB, %5.2f TB/s, %5.2f x HBM time  -> %d'
                         % (L['kind'] + (' dual' if L['nhalves'] == 2 else ''), L['K'], L['M'], m14, min(r[i]['ms'] for r in b), max(r[i]['ms'] for r in b), m1, m2, spread,
                            m13 / m14, bytes_ / 1e6, bytes_ / (m14 * 1e-3) / 1e12, m14 / t_hbm, 14 if m14 < m13 - spread else 13))
        if stride == 2:
            lines.append('    phases summed: cfg 14 %.4f ms, cfg 13 %.4f ms' % (tot[14], tot[13]))
    if not args.no_net:
        from xfr_amd.models import mobilenet, whitebox as WB
        bb = mobilenet.mobilenet_v1(num_classes=16).to(dev)
        wbn = WB.WhiteboxTVResnet(bb)
        wb = WB.Whitebox(wbn)
        g = torch.Generator().manual_seed(5)
        x = torch.randn((BATCH, 3, 224, 224), generator=g).to(dev)
        xm = torch.randn((BATCH, bb.feature_dim), generator=g).to(dev) / 2500
        xn = torch.randn((BATCH, bb.feature_dim), generator=g).to(dev) / 2500
        wb.contrastive_triplet_ebp_batch(x, xm, xn)
        torch.cuda.synchronize()
        eng = wbn.engine(BATCH)
        res = {13: [], 14: []}
        for _ in range(3):
            for cfg in (14, 13):
                eng.set_epilogue_fusion(3 | (KEEP_ON_13 if cfg == 13 else 0))
                wb.contrastive_triplet_ebp_batch(x, xm, xn)
                torch.cuda.synchronize()
                ts = []
                for _ in range(args.rounds):
                    t0 = time.perf_counter()
                    out = wb.contrastive_triplet_ebp_batch(x, xm, xn)
                    torch.cuda.synchronize()
                    ts.append(time.perf_counter() - t0)
                assert bool(torch.isfinite(torch.as_tensor(out)).all())
                res[cfg].append(BATCH / med(ts))
        for cfg in (14, 13):
            lines.append('mobilenet.mobilenet_v1, 224 x 224, contrastive_triplet_ebp_batch at batch %d (seeded random weights and images; host clock around synchronised calls; '
                         'three runs, each the median of %d calls), depthwise launches on configuration %d: %s maps/s'
                         % (BATCH, args.rounds, cfg, ', '.join('%.1f' % v for v in res[cfg])))
        eng.close()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
