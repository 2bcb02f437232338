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

--black-box whitebox --model resnet101|resnet50_128|lightcnn measures the generator's black box instead (WhiteboxBlackBox: every masked probe
through the uint8 of convert_from_numpy and the network's own preprocess; xfr_strise_score_ex with quantize = 1), alternating in one process:

* forward_only_seconds / quant_sweep_seconds, and on resnet101 named_sweep_seconds (xfr_strise_score of the same engine): medians of --rounds;
* quant_vs_forward_only, and on resnet101 quant_vs_named (named sweep time over quantised sweep time);
* generate_ms_per_batch   the generate kernel of one batch alone through the parity hook, timed on the host: argument marshalling, the pageable
  table upload, a stream synchronisation and the output's allocation are in it, so it is an upper bound of the kernel and, where it is a
  fraction of a millisecond, mostly that overhead; next to forward_ms_per_batch.

    python tools/strise_probe.py --black-box whitebox --model lightcnn --masks 6500 --batch 128 --rounds 7
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


def main_whitebox(args):
    import numpy as np
    import torch
    from xfr_amd import synth
    from xfr_amd.models import blackbox as BB
    from xfr_amd.models import lightcnn, resnet, resnet50_128, whitebox as WB

    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    if args.model == 'resnet101':
        bb, wrap = resnet.ResNet([3, 4, 23, 3], num_classes=2), WB.WhiteboxSTResnet
    elif args.model == 'resnet50_128':
        bb, wrap = resnet50_128.Resnet50_128(), WB.Whitebox_resnet50_128
    else:
        bb, wrap = lightcnn.LightCNN_29Layers_v2(num_classes=2), WB.WhiteboxLightCNN
    bb.load_state_dict(synth.synth_state_dict(bb, seed=0))
    bb.to(dev)
    wbn = wrap(bb)
    wbn.default_max_batch = args.batch
    wb = WB.Whitebox(wbn)
    wb.batch_size = args.batch
    box = BB.WhiteboxBlackBox(wb)
    base = synth.synth_smooth_images(3, (3, 224, 224), seed=1)
    u8 = lambda t: t.permute(1, 2, 0).numpy().astype(np.uint8)                     # noqa: E731
    g = torch.Generator().manual_seed(3)
    gallery = [u8(torch.floor(0.8 * base[2] + 51.0 * torch.rand((3, 224, 224), generator=g))) for _ in range(args.gallery)]
    st = BB.STRise(probe=u8(base[0]), refs=[u8(base[1])], gallery=gallery, black_box_fn=box, prior_type='uniform', num_masks=args.masks,
                   num_mask_elements=args.elements)
    np.random.seed(0)
    st.uniform_prior()
    st.generate_masks()
    st.apply_masks()
    ok, tables = box.device_route(st.probe, st.fill_image)
    assert ok, tables
    eng, enc = wb._engine(args.batch), wb.net._mark('encode')
    refs, gal = box.embed_raw(st.refs), box.embed_raw(st.gallery)
    probe, fill = torch.from_numpy(st.probe).to(dev), torch.from_numpy(st.fill_image).to(dev)
    cells, shifts, grid, scale = st._mask_args()
    n_batches = (args.masks + 1 + args.batch - 1) // args.batch
    quant = dict(probe_shape=(224, 224), quantize=True, tables=tables)

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()

    def generate():
        return eng.strise_masked_probes(probe, fill, cells, shifts, grid, scale, 0, min(args.batch, args.masks), **quant)
    resident = generate()
    if resident.shape[0] < args.batch:
        resident = resident.repeat((args.batch + resident.shape[0] - 1) // resident.shape[0], 1, 1, 1)[:args.batch].contiguous()
    named = args.model == 'resnet101'
    eng.strise_score(probe, fill, cells, shifts, grid, scale, refs, gal, enc, **quant)      # warm-up: streams, buffers, clocks
    fwd, sweep, old, gen = [], [], [], []
    for _ in range(max(1, args.rounds)):
        t0 = sync()
        for _ in range(n_batches):
            wb.encode(resident)
        fwd.append(sync() - t0)
        t0 = sync()
        scores, _ = eng.strise_score(probe, fill, cells, shifts, grid, scale, refs, gal, enc, **quant)
        sweep.append(sync() - t0)
        if named:
            t0 = sync()
            eng.strise_score(probe, fill, cells, shifts, grid, scale, refs, gal, enc)
            old.append(sync() - t0)
        t0 = sync()
        generate()
        gen.append(sync() - t0)
    med = lambda v: sorted(v)[len(v) // 2]                                          # noqa: E731
    out = {'workload': 'STRise sweep behind WhiteboxBlackBox, %s, synthetic' % args.model, 'masks': args.masks, 'batch': args.batch, 'gallery': args.gallery,
           'elements': args.elements, 'batches': n_batches, 'quant_sweep_seconds': med(sweep), 'forward_only_seconds': med(fwd),
           'quant_vs_forward_only': med(fwd) / med(sweep), 'quant_sweep_masks_per_s': args.masks / med(sweep),
           'generate_ms_per_batch': 1e3 * med(gen), 'forward_ms_per_batch': 1e3 * med(fwd) / n_batches,
           'generate_includes': 'host-timed parity hook: marshalling, table upload, stream synchronisation, allocation -- an upper bound of the kernel',
           'scores_finite': bool(np.isfinite(scores.cpu().numpy()).all()), 'quant_sweeps_seconds': sweep, 'forward_only_all_seconds': fwd,
           'generate_all_seconds': gen, 'reported': 'medians of %d alternating rounds in one process' % len(sweep)}
    if named:
        out.update({'named_sweep_seconds': med(old), 'quant_vs_named': med(old) / med(sweep), 'named_sweeps_seconds': old})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--black-box', choices=('named', 'whitebox'), default='named')
    ap.add_argument('--model', choices=('resnet101', 'resnet50_128', 'lightcnn'), default='resnet101')
    ap.add_argument('--masks', type=int, default=6500)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--gallery', type=int, default=50)
    ap.add_argument('--elements', type=int, default=1)
    ap.add_argument('--rounds', type=int, default=3, help='alternating (forward-only, sweep) pairs; medians are reported')
    args = ap.parse_args()
    if args.black_box == 'whitebox':
        return main_whitebox(args)
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
