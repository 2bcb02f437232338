#!/usr/bin/env python
"""Image intake on synthetic weights and synthetic crops (xfr_amd/intake.py, csrc/intake.hip): 256 uint8 crops whose sides are
drawn by a fixed seed from [96, 640], ResNet-101, every figure the median of --rounds rounds in which the variants alternate, each ending in a
device synchronise, after one untimed round.

  1. the device intake from host memory -- the crops packed into one buffer, uploaded and resized (xfr_intake_u8_host) -- and from a buffer that is
     on the device already (xfr_intake_u8), in images/s;
  2. the host chain on the same crops as its callers run it, one image at a time (Whitebox.convert_from_numpy);
  3. the forward alone on the resulting uint8 batch (encode_u8 in chunks of --batch);
  4. embeddings(arrays) end to end: intake 'auto' against the host chain in front of the same forward (what embeddings does with intake='host', and
     what the callers of the parent did: convert_from_numpy per image, then embeddings), and whether the bytes and the encodings agree.

    python tools/intake_probe.py [--crops 256] [--batch 128] [--rounds 5] [--out profiles/r15/intake_probe.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--crops', type=int, default=256)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-rounds', type=int, default=3, help='rounds of the two variants that run the host chain')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r15', 'intake_probe.txt'))
    args = ap.parse_args()
    import numpy as np
    import torch
    from xfr_amd import intake, synth
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
    eng = wbn.engine(args.batch)

    rs = np.random.RandomState(15)
    sides = rs.randint(96, 641, size=args.crops)
    crops = [rs.randint(0, 256, size=(s, s, 3)).astype(np.uint8) for s in sides]
    items = [(c, intake.HEAD_F32) for c in crops]
    out_hw = (224, 224)
    n = args.crops

    src, table = intake.pack(items)
    src_dev = torch.from_numpy(src).to(dev)
    eng.intake_set_kernels(*intake.stated_kernels(items, out_hw))
    u8 = eng.intake_u8(src_dev, table, out_hw)

    variants = {
        'intake_host': (lambda: intake.device_bytes(eng, items, out_hw), args.rounds),
        'intake_upload': (lambda: eng.intake_u8(src, table, out_hw), args.rounds),
        'intake_dev': (lambda: eng.intake_u8(src_dev, table, out_hw), args.rounds),
        'forward': (lambda: [wbn.encode_u8(b) for b in torch.split(u8, args.batch)], args.rounds),
        'e2e_auto': (lambda: wb.embeddings(crops, norm=False, intake='auto'), args.rounds),
        'host_chain': (lambda: [wb.convert_from_numpy(c)[0] for c in crops], args.host_rounds),
        'e2e_host': (lambda: wb.embeddings([wb.convert_from_numpy(c)[0] for c in crops], norm=False), args.host_rounds),
    }
    times = {k: [] for k in variants}
    last = {}
    for r in range(-1, max(args.rounds, args.host_rounds)):
        for name, (fn, rounds) in variants.items():
            if r >= rounds:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            if r >= 0:
                times[name].append(time.perf_counter() - t0)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}

    bytes_dev = last['intake_host'].cpu().numpy()
    k = min(16, n)
    bytes_ok = all(np.array_equal(bytes_dev[i], intake.host_bytes(crops[i], out_hw, intake.HEAD_F32)) for i in range(k))
    same_bytes = np.array_equal(bytes_dev, last['intake_dev'].cpu().numpy()) and np.array_equal(bytes_dev, last['intake_upload'].cpu().numpy())
    enc_equal = np.array_equal(last['e2e_auto'], last['e2e_host'])
    lines = [
        'intake_probe: %d crops, sides %d..%d (median %d), %.1f MB of uint8 sources, to 224 x 224; ResNet-101 (synthetic), chunks of %d; medians of %d '
        'alternating rounds (%d for the host chain)' % (n, sides.min(), sides.max(), int(np.median(sides)), src.size / 1e6, args.batch, args.rounds, args.host_rounds),
        'device intake, host memory, packing included (intake.device_bytes): %.1f ms, %.0f images/s' % (med['intake_host'] * 1e3, n / med['intake_host']),
        'device intake, host memory, packed already (xfr_intake_u8_host):    %.1f ms, %.0f images/s' % (med['intake_upload'] * 1e3, n / med['intake_upload']),
        'device intake, device memory (xfr_intake_u8):                       %.1f ms, %.0f images/s' % (med['intake_dev'] * 1e3, n / med['intake_dev']),
        'host chain, one image at a time (convert_from_numpy):               %.1f ms, %.0f images/s' % (med['host_chain'] * 1e3, n / med['host_chain']),
        'forward alone on the uint8 batch (encode_u8):                       %.1f ms, %.0f images/s' % (med['forward'] * 1e3, n / med['forward']),
        'embeddings(arrays) end to end, intake auto:                         %.1f ms, %.0f images/s' % (med['e2e_auto'] * 1e3, n / med['e2e_auto']),
        'embeddings behind the host chain (intake host, the parent):         %.1f ms, %.0f images/s' % (med['e2e_host'] * 1e3, n / med['e2e_host']),
        'bytes: the first %d crops equal host_bytes: %s; the three device variants agree: %s; the encodings of the two end-to-end paths are equal: %s'
        % (k, bytes_ok, same_bytes, enc_equal),
        'device intake from host memory / forward alone: %.2f (target: at most 1)' % (med['intake_host'] / med['forward']),
    ]
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)
    if not (bytes_ok and same_bytes and enc_equal):
        sys.exit(1)


if __name__ == '__main__':
    main()
