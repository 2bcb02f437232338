#!/usr/bin/env python
"""Error of the GEMM kernels against a float64 convolution (CPU): RMS and mean signed error of the fp32 MFMA kernels (cfg 4, 7) and the bf16x6 kernel
(cfg 9) on deep-K layer shapes, with post-ReLU-like (half zero, non-negative) and signed inputs.   python tools/conv_error_probe.py"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--extra', action='store_true', help='also odd K-step counts, M tails, relu on the input, tiny and large grids (whole tiles and stream-K shares)')
    ap.add_argument('--cfgs', default='4,7,9')
    ap.add_argument('--lean', action='store_true', help='the lean two-accumulator launches (xfr_debug_conv cfg + 100) at the 1x1 shapes of the ResNet-101 step: '
                                                        'the W tile and the stored quotient against float64')
    args = ap.parse_args()
    import numpy as np
    import torch
    from xfr_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda', 0)
    torch.set_num_threads(16)
    if args.lean:
        return lean(args, np, torch, _lib, lib, dev)
    shapes = [(256, 14, 14, 8, 256, 3, 1, 0), (1024, 14, 14, 8, 256, 1, 0, 0), (128, 28, 28, 4, 128, 3, 1, 0)]
    if args.extra:       # (.., relu_in)
        shapes += [(48, 20, 20, 2, 128, 3, 1, 0), (64, 14, 14, 3, 128, 3, 1, 1), (16, 15, 15, 5, 256, 5, 2, 0), (1024, 14, 14, 64, 256, 1, 0, 0),
                   (256, 14, 14, 1, 256, 3, 1, 0), (256, 14, 14, 64, 256, 3, 1, 0), (128, 28, 28, 66, 128, 3, 1, 1), (2048, 14, 14, 2, 512, 1, 0, 0)]
    for (cin, h, w, nb, cout, k, pad, relu_in) in shapes:
        for kind in (('relu', 'signed', 'wide') if not relu_in else ('signed',)):
            g = torch.Generator().manual_seed(1)
            x = torch.randn((nb, cin, h, w), generator=g, dtype=torch.float64)
            if kind == 'relu':
                x = x.clamp_min(0)
            if kind == 'wide':            # gradient-like: magnitudes over many decades
                x = x * torch.exp(8 * torch.randn((nb, cin, h, w), generator=g, dtype=torch.float64))
            x = x.float()
            xin = x.clamp_min(0) if relu_in else x
            wt = (torch.randn((cout, cin, k, k), generator=g) / (cin * k * k) ** 0.5).contiguous()
            want = torch.nn.functional.conv2d(xin.double(), wt.double(), None, padding=pad)
            mag = torch.nn.functional.conv2d(xin.double().abs(), wt.double().abs(), None, padding=pad)       # sum of |terms|
            xg = x.to(dev).permute(1, 0, 2, 3).contiguous()
            line = '%-30s %-6s' % ((cin, h, nb, cout, k, relu_in), kind)
            for cfg in [int(c) for c in args.cfgs.split(',')]:
                out = torch.zeros((cout, nb) + tuple(want.shape[2:]), device=dev)
                ms = ctypes.c_float()
                _lib.check(lib.xfr_debug_conv(xg.data_ptr(), wt.data_ptr(), None, out.data_ptr(), cin, h, w, nb, cout, k, k, 1, pad, relu_in, cfg, 1, ctypes.byref(ms)))
                got = out.permute(1, 0, 2, 3).cpu().double()
                e = (got - want) / mag
                line += ' | cfg %d: rms %.2e mean %+.2e max %.2e' % (cfg, float(e.pow(2).mean().sqrt()), float(e.mean()), float(e.abs().max()))
            print(line, flush=True)


def lean(args, np, torch, _lib, lib, dev):
    """Lean probe-forward launches: g = relu(conv(W, x)) as (got - want) / sum of |terms|, like the rows above; the relu(W) tile through what the
    launch stores of it, q = g / (conv(relu W, x) + eps): (|q| - q64) / q64 over the elements with g > 0 (both kernels round the same last division),
    and how many sign bits (g <= 0) differ from float64's.  Inputs are post-ReLU-like (half zero, non-negative)."""
    # cin, h, w, nb, cout: 1024 <- 256 at M = 6272, 2048 <- 512 at M = 1568, 128 <- 512 at M = 25088, and a shallow two-pass layer with an M tail
    shapes = [(256, 14, 14, 32, 1024), (512, 7, 7, 32, 2048), (512, 28, 28, 32, 128), (96, 7, 7, 4, 256)]
    eps = 1e-16
    for (cin, h, w, nb, cout) in shapes:
        g = torch.Generator().manual_seed(1)
        x = torch.randn((nb, cin, h, w), generator=g, dtype=torch.float64).clamp_min(0).float()
        wt = (torch.randn((cout, cin, 1, 1), generator=g) / cin ** 0.5).contiguous()
        raw = torch.nn.functional.conv2d(x.double(), wt.double())
        mag = torch.nn.functional.conv2d(x.double(), wt.double().abs())
        pos = torch.nn.functional.conv2d(x.double(), wt.double().clamp_min(0))
        want_g = raw.clamp_min(0)
        want_q = want_g / (pos + eps)
        live = raw > 1e-6 * mag                # away from the ReLU's edge: a sign flip there is a tie, not an error
        xg = x.to(dev).permute(1, 0, 2, 3).contiguous()
        line = '%-28s' % ((cin, h, nb, cout),)
        for cfg in [int(c) for c in args.cfgs.split(',')]:
            out = torch.full((2, cout, nb, h, w), float('nan'), device=dev)
            ms = ctypes.c_float()
            _lib.check(lib.xfr_debug_conv(xg.data_ptr(), wt.data_ptr(), None, out.data_ptr(), cin, h, w, nb, cout, 1, 1, 1, 0, 0, 100 + cfg, 1, ctypes.byref(ms)))
            got = out.permute(0, 2, 1, 3, 4).cpu()
            got_g, got_q = got[0].double(), got[1]
            sign = (got_q.view(torch.int32) < 0)
            e = (got_g - want_g) / mag
            eq = ((got_q.abs().double() - want_q) / want_q)[live]
            line += ' | cfg %d: g rms %.2e mean %+.2e max %.2e; q rms %.2e mean %+.2e max %.2e; sign bits off %d' % (
                cfg, float(e.pow(2).mean().sqrt()), float(e.mean()), float(e.abs().max()), float(eq.pow(2).mean().sqrt()), float(eq.mean()), float(eq.abs().max()),
                int((sign[live] != (raw[live] <= 0)).sum()))
        print(line, flush=True)


if __name__ == '__main__':
    main()
