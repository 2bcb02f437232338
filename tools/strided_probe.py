#!/usr/bin/env python
"""The backward-data pass of a strided 3x3 convolution by phases, against what zero insertion would run.

For the 3x3 / stride 2 / pad 1 layers of ResNet-50 v1.5 at batch 32 (C -> C channels, H x H -> H/2 x H/2), one gradient stream, GEMM times from
the engine's per-launch profile (events around every launch), fp32 MFMA kernels throughout (bf16x6 off), epilogue fusion off so that all three
are plain GEMM launches with their chains in kernels of their own:

  (a) the four phase launches of the strided layer's backward-data pass, summed (the zero fill in front of them is not a GEMM and not included);
  (b) the stride-1 3x3 backward-data launch of the same channels at the INPUT resolution: what zero insertion would run;
  (c) the same launch at the OUTPUT resolution: the same algorithmic FLOPs as (a).

--rounds alternating rounds (a, b, c per shape), medians.  Gate: (a) < (b) on every shape, else exit status 1; (a) / (c) is reported only.
The profile times launches one by one, so (a) is the phases in a row; the engine runs them side by side on side streams (backward.hip), and the
un-profiled wall time of a whole sweep with and without that (fusion-mask bit 9) is reported next to it.
Then maps/s of tv_resnet [3, 4, 6, 3] v1.5 through Whitebox.contrastive_triplet_ebp_batch at batch 32 (reported only).

    python tools/strided_probe.py [--rounds 7] [--out profiles/r18/strided_probe.txt]
"""
import argparse
import csv
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((128, 56), (256, 28), (512, 14))
BATCH = 32


def _program(c, h, stride):
    """conv 1x1 C -> C, ReLU, conv 3x3 C -> C with the given stride, ReLU, global average pool, Linear: the 3x3's backward-data pass is timed."""
    from xfr_amd.program import Program
    p = Program((c, h, h))
    t = p.relu_(p.conv(0, 'conv0', c, 1, bias=False))
    t = p.relu_(p.conv(t, 'conv1', c, 3, stride=stride, pad=1, bias=False))
    ho = (h + 2 - 3) // stride + 1
    t = p.avgpool(t, ho, 1)
    return p, p.mark('classify', p.linear(t, 'fc', 8, (1, 1), bias=False))


def _weights(c):
    import torch
    g = torch.Generator().manual_seed(c)
    return {'conv0.weight': torch.randn((c, c, 1, 1), generator=g) / c ** 0.5, 'conv1.weight': torch.randn((c, c, 3, 3), generator=g) / (9 * c) ** 0.5,
            'fc.weight': torch.randn((8, c), generator=g) / c ** 0.5}


class _Leg(object):
    """One engine and its inputs; run() -> milliseconds of the 3x3's backward-data GEMM launches of one sweep."""

    def __init__(self, c, h, stride, dev, csv_path):
        import torch
        from xfr_amd.engine import Engine
        prog, self.st = _program(c, h, stride)
        self.eng = Engine(prog, BATCH, dev)
        self.eng.load_weights(_weights(c))
        self.eng.set_mode('affineonly_with_prior')
        self.eng.set_split_gemm(0)
        self.eng.set_epilogue_fusion(0)
        self.eng.set_lean(0)
        g = torch.Generator().manual_seed(h)
        self.x = torch.randn((BATCH, c, h, h), generator=g).to(dev)
        self.seed = torch.rand((1, BATCH, 8), generator=g).to(dev)
        self.stride, self.c, self.csv = stride, c, csv_path
        self.eng.ebp(self.x, self.st, self.seed)          # untimed: allocations, first launches
        self.eng.set_profile(True)

    def run(self):
        import torch
        if os.path.exists(self.csv):
            os.remove(self.csv)
        self.eng.profile_csv(self.csv)
        self.eng.ebp(self.x, self.st, self.seed)
        torch.cuda.synchronize()
        self.eng.profile_csv(None)
        with open(self.csv) as f:
            rows = [r for r in csv.reader(f)]
        # columns: Cout, nhalves, K, M, kh, stride, out_stride, relu_in, accumulate, ms, TFLOP/s, cfg
        if self.stride == 2:
            mine = [r for r in rows if int(r[6]) == 2]
            assert len(mine) == 4, rows
        else:
            mine = [r for r in rows if int(r[4]) == 3 and int(r[2]) == 9 * self.c][-1:]          # forward first, backward last
            assert len(mine) == 1, rows
        return sum(float(r[9]) for r in mine), [(int(r[2]), int(r[3]), int(r[11])) for r in mine]

    def wall(self, in_a_row, calls=20):
        """Milliseconds per un-profiled sweep (forward and backward of the whole three-layer net), the phases side by side or in a row."""
        import torch
        self.eng.set_profile(False)
        self.eng.set_epilogue_fusion(512 if in_a_row else 0)          # bit 9: the phase launches one after another
        self.eng.ebp(self.x, self.st, self.seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            self.eng.ebp(self.x, self.st, self.seed)
        torch.cuda.synchronize()
        self.eng.set_epilogue_fusion(0)
        self.eng.set_profile(True)
        return (time.perf_counter() - t0) / calls * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r18', 'strided_probe.txt'))
    ap.add_argument('--no-net', action='store_true', help='skip the tv_resnet throughput')
    args = ap.parse_args()
    import torch
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    tmp = tempfile.mkdtemp()
    med = lambda t: sorted(t)[len(t) // 2]      # noqa: E731
    lines = ['strided_probe: 3x3 / stride 2 / pad 1 backward-data at batch %d, one gradient stream, fp32 MFMA kernels, epilogue fusion off; medians of %d alternating rounds'
             % (BATCH, args.rounds),
             '(a) four phase launches summed  (b) stride-1 3x3 at the input resolution (zero insertion)  (c) stride-1 3x3 at the output resolution (equal FLOPs)',
             'gated: (a) < (b) on every shape.  reported, not gated: (a) / (c), the maps/s below.']
    ok = True
    for c, h in SHAPES:
        legs = [_Leg(c, h, 2, dev, os.path.join(tmp, 'a.csv')), _Leg(c, h, 1, dev, os.path.join(tmp, 'b.csv')), _Leg(c, h // 2, 1, dev, os.path.join(tmp, 'c.csv'))]
        t = [[], [], []]
        info = [None, None, None]
        for _ in range(args.rounds):
            for i, leg in enumerate(legs):
                ms, info[i] = leg.run()
                t[i].append(ms)
        a, b, cc = med(t[0]), med(t[1]), med(t[2])
        ok = ok and a < b
        lines.append('%3d -> %3d  %2d^2 -> %2d^2   (a) %.4f ms (rounds %.4f .. %.4f)   (b) %.4f ms   (c) %.4f ms   (a)/(b) %.3f  (a)/(c) %.3f   %s'
                     % (c, c, h, h // 2, a, min(t[0]), max(t[0]), b, cc, a / b, a / cc, 'ok' if a < b else 'FAIL: the phases are not faster than zero insertion'))
        lines.append('            phase launches (K, M, cfg): %s;  (b) %s  (c) %s' % (info[0], info[1], info[2]))
        w = [[], []]
        for _ in range(args.rounds):
            for i in (0, 1):
                w[i].append(legs[0].wall(i == 1))
        lines.append('            whole sweep of the strided net, un-profiled wall time: phases side by side %.4f ms, in a row %.4f ms (difference %.4f ms; reported, not gated)'
                     % (med(w[0]), med(w[1]), med(w[1]) - med(w[0])))
        for leg in legs:
            leg.eng.close()
    if not args.no_net:
        from xfr_amd.models import tv_resnet, whitebox as WB
        bb = tv_resnet.resnet50(num_classes=16).to(dev)
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
        lines.append('tv_resnet [3, 4, 6, 3] v1.5, 224 x 224, contrastive_triplet_ebp_batch at batch %d (seeded random weights and images): %.1f ms per call '
                     '(rounds %.1f .. %.1f), %.1f maps/s' % (BATCH, med(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3, BATCH / med(ts)))
        wbn.engine().close()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
