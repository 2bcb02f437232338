#!/usr/bin/env python
"""Saliency finishing, device against host (xfr_finish_saliency, xfr_amd/csrc/finish.hip): --maps maps of 112 x 112 finished to
224 x 224 with overlays, in maps/s.

  device   Engine.finish_saliency on device-resident maps and probes, then both results copied to the host (what save_finished needs), ending in a
           device synchronise: one untimed call, then --repeat rounds of --calls calls each; the median round and the spread of the rounds;
  host     the chain create_save_smap runs per map (float32 head, processSaliency, blend_saliency_map, the uint8 conversion) on the same maps, one
           process per CPU the machine grants (--cpus, default: the scheduler's affinity count capped at 16), the same rounds.
The two alternate, round by round.  The distances of the device results from the host's own are printed per shape: the map against the chain with the
float32 nearest to the exact sum (the device's own total) and against the unmodified chain, r (the reference's distance from itself), and the overlay
pixels that differ.

    python tools/finish_probe.py [--maps 32] [--repeat 7] [--calls 20]
"""
import argparse
import multiprocessing
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _host_one(args):
    import finish_inputs as F
    return F.host_chain(*args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--maps', type=int, default=32)
    ap.add_argument('--repeat', type=int, default=7)
    ap.add_argument('--calls', type=int, default=20, help='device calls per timed round')
    ap.add_argument('--cpus', type=int, default=0)
    args = ap.parse_args()
    import numpy as np
    import torch
    import finish_inputs as F
    from xfr_amd.engine import Engine
    from xfr_amd.models import resnet

    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    eng = Engine(resnet.ResNet([1, 1, 1, 1], num_classes=5).build_program(), 1, dev)      # the engine lends its device: no weights
    cpus = args.cpus or min(16, len(os.sched_getaffinity(0)))
    n = args.maps
    maps = np.stack([F.seeded_map('field', (112, 112), i) for i in range(n)])
    probes = np.stack([F.seeded_probe((224, 224), i) for i in range(n)])
    dm, dp = torch.from_numpy(maps).to(dev), torch.from_numpy(probes).to(dev)

    def device_round():
        t0 = time.perf_counter()
        for _ in range(args.calls):
            sal, ov = eng.finish_saliency(dm, (224, 224), probes_u8=dp)
            out = sal.cpu(), ov.cpu()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.calls, out

    pool = multiprocessing.get_context('spawn').Pool(cpus)      # spawn: the children never see this process's device

    def host_round():
        t0 = time.perf_counter()
        out = pool.map(_host_one, list(zip(maps, probes)))
        return time.perf_counter() - t0, out

    device_round()
    host_round()
    td, th = [], []
    for _ in range(args.repeat):
        td.append(device_round()[0])
        th.append(host_round()[0])
    pool.close()
    pool.join()
    med = lambda t: sorted(t)[len(t) // 2]      # noqa: E731
    print('device finish: %d maps 112 x 112 -> 224 x 224 with overlays, results on the host: %.3f ms per call (rounds %.3f .. %.3f), %.0f maps/s'
          % (n, med(td) * 1e3, min(td) * 1e3, max(td) * 1e3, n / med(td)), flush=True)
    print('host chain:    the same maps on %d CPUs: %.1f ms per batch (rounds %.1f .. %.1f), %.0f maps/s; device / host = %.1f x'
          % (cpus, med(th) * 1e3, min(th) * 1e3, max(th) * 1e3, n / med(th), med(th) / med(td)), flush=True)

    r = F.reference_r()
    print('r (host_chain against host_chain_exact_total, 3 maps of every varying shape) = %.3e' % r)
    for name in F.CASES:
        m, p = F.batch(name, 3)
        sal, ov = eng.finish_saliency(torch.from_numpy(m.copy()), F.CASES[name][2], probes_u8=torch.from_numpy(p.copy()))
        sal, ov = sal.cpu().numpy(), ov.cpu().numpy()
        exact, plain = F.truth(name, 3, True), F.truth(name, 3, False)
        differ = max(int((ov[i] != exact[1][i]).any(axis=-1).sum()) for i in range(3))
        print('%-20s %9s -> %-9s  map against exact-total chain %.3e, against host_chain %.3e; overlay: at most %d of %d pixels differ'
              % (name, '%d x %d' % F.CASES[name][1], '%d x %d' % F.CASES[name][2], np.abs(sal - exact[0]).max(), np.abs(sal - plain[0]).max(),
                 differ, sal[0].size))


if __name__ == '__main__':
    main()
