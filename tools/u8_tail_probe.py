#!/usr/bin/env python
"""What the device tail of ebp_version != 6 (xfr_mwp_to_saliency_u8, output 'uint8_saliency') buys over the host chain it replaces.
    python tools/u8_tail_probe.py [--maps 64] [--n 8] [--topk 32] [--rounds 5] [--out FILE]
1. `--maps` float32 maps of 112 x 112 on the device -> uint8 saliency maps on the host: Engine.mwp_to_saliency_u8 plus the copy of the bytes,
   against the device-to-host copy of the floats plus Whitebox._mwp_to_saliency's host branch (NumPy stretch, Pillow blur, NumPy stretch) map by map.
2. The weighted-subtree probe of tools/subtree_probe.py --native (ResNet-101, 'norelu', `--n` probes, top-`--topk`) at ebp_version 7, ms per probe:
   the native call with output 'uint8_saliency', against the same call as the parent commit made it -- output 'uint8', the merged map and the top-k
   maps copied down, topk + 1 Pillow blurs per probe (restated below as `_parent_native`; the engine calls of that path are untouched).
Both legs of a comparison run in the same process, alternating, `--rounds` times; the median, the minimum and the maximum of the rounds are printed,
and the bytes of the two legs are compared.  Needs a HIP device; there is no CPU path."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, reps):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / reps, r


def _ab(legs, rounds, reps):
    """legs: [(name, fn)].  Alternates them `rounds` times -> {name: [ms per call of every round]}, {name: last result}."""
    ms, last = {k: [] for k, _ in legs}, {}
    for k, fn in legs:
        fn()                       # warm
    for _ in range(rounds):
        for (k, fn), r in zip(legs, reps):
            t, last[k] = _timed(fn, r)
            ms[k].append(t)
    return ms, last


def _line(name, v, per=1, unit='ms'):
    v = [x / per for x in v]
    return '  %-46s median %9.3f  min %9.3f  max %9.3f %s  (%d rounds)' % (name, statistics.median(v), min(v), max(v), unit, len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--maps', type=int, default=64)
    ap.add_argument('--n', type=int, default=8)
    ap.add_argument('--topk', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--max-batch', type=int, default=128)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r17', 'u8_tail_probe.txt'))
    args = ap.parse_args()
    import numpy as np
    import torch
    from xfr_amd import synth
    from xfr_amd.inpainting_game import SUBTREE_VERSIONS
    from xfr_amd.models import resnet, whitebox as WB
    if not torch.cuda.is_available():
        sys.exit('u8_tail_probe: no HIP device visible; there is nothing to measure on a CPU')
    dev = torch.device('cuda', 0)
    bb = resnet.ResNet([3, 4, 23, 3], num_classes=2)
    bb.load_state_dict(synth.synth_state_dict(bb, seed=0))
    bb.to(dev)
    wbn = WB.WhiteboxSTResnet(bb)
    wbn.default_max_batch = args.max_batch
    wb = WB.Whitebox(wbn, ebp_version=7, ebp_subtree_mode='norelu')
    eng = wb._engine(args.n)
    lines = ['u8_tail_probe: %s, %d rounds, the two legs of each comparison alternating in one process' % (torch.cuda.get_device_name(0), args.rounds)]

    # 1. the tail alone
    rng = np.random.RandomState(5)
    maps = torch.as_tensor((rng.rand(args.maps, 112, 112) ** 4).astype(np.float32)).to(dev)
    device_tail = lambda: eng.mwp_to_saliency_u8(maps).cpu().numpy()                                          # noqa: E731
    host_chain = lambda: np.stack([wb._mwp_to_saliency(m) for m in maps.cpu().numpy()])                       # noqa: E731
    ms, last = _ab([('device', device_tail), ('host', host_chain)], args.rounds, (50, 3))
    same = bool(np.array_equal(last['device'], last['host']))
    lines += ['1. %d maps 112 x 112, float32 on the device -> uint8 on the host, ms per call (bytes equal: %s)' % (args.maps, same),
              _line('device tail + copy of the bytes', ms['device']),
              _line('copy of the floats + NumPy / Pillow per map', ms['host']),
              '  ratio of the medians: %.1f x' % (statistics.median(ms['host']) / statistics.median(ms['device']))]

    # 2. the weighted-subtree probe at ebp_version 7
    n = args.n
    x = synth.synth_smooth_images(n, (3, 224, 224), seed=3, mean=resnet.MEAN_RGB).to(dev)
    xm, xn = synth.unit_rows(n, 512, seed=1).to(dev), synth.unit_rows(n, 512, seed=2).to(dev)
    do_max, gating = SUBTREE_VERSIONS[7]
    st = wb.net._program.marks['encode']

    def new_native():
        return wb.weighted_subtree_ebp_batch(x, xm, xn, topk=args.topk, do_max_subtree=do_max, do_mated_similarity_gating=gating, native=True)

    def _parent_native():
        """_weighted_subtree_native as the parent commit had it: levels from the engine, the blurs on the host."""
        eng_ = wb._engine(n)
        xd, _ = eng_._prep(x)
        seeds = torch.stack([v.reshape(n, -1) for v in (xm, xn, xm)], dim=0)
        smap, top, w_valid, k_valid, n_valid = eng_.weighted_subtree(xd, st, seeds, args.topk, gate_ge0=gating, do_max_subtree=do_max, output='uint8',
                                                                     order='numpy')
        smap, top = smap.cpu().numpy(), top.cpu().numpy()
        res = []
        for b in range(n):
            k = int(n_valid[b])
            res.append((wb._mwp_to_saliency(smap[b].astype(np.uint8)), [wb._mwp_to_saliency(top[b, i]) for i in range(k)],
                        [float(v) for v in w_valid[b, :k]], [int(v) for v in k_valid[b, :k]]))
        return res

    wb._ebp_subtree_mode = 'norelu'
    ms, last = _ab([('new', new_native), ('parent', _parent_native)], args.rounds, (2, 2))
    same = all(np.array_equal(a[0], b[0]) and a[3] == b[3] and all(np.array_equal(p, q) for p, q in zip(a[1], b[1]))
               for a, b in zip(last['new'], last['parent']))
    lines += ['2. weighted subtree EBP, ResNet-101 norelu, ebp_version 7, %d probes, top-%d, native call, ms per probe (maps and selections equal: %s; '
              'valid subtrees %s)' % (n, args.topk, same, [len(r[3]) for r in last['new']]),
              _line("output 'uint8_saliency' (this commit)", ms['new'], n),
              _line("output 'uint8' + host blurs (the parent's path)", ms['parent'], n),
              '  difference of the medians: %.3f ms per probe' % ((statistics.median(ms['parent']) - statistics.median(ms['new'])) / n)]
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write(text)


if __name__ == '__main__':
    main()
