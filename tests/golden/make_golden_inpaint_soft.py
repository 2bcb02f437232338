#!/usr/bin/env python
"""Golden vectors for soft-edged masks (mask_blur_sigma) and 'percent-pixels' levels of inpainting-game scoring
(python/xfr/inpainting_game/inpainting_game.py:57-75), produced by the REAL reference functions on the CPU.
Usage: python tests/golden/make_golden_inpaint_soft.py  ->  tests/golden/golden_inpaint_soft.npz

It follows make_golden_inpaint_game.py, whose Double wrapper and percent-density conditions it imports: the reference is loaded unchanged through
ref_import.load() (skimage.filters.gaussian is that file's scipy restatement).  Inputs are tests/inpaint_soft_inputs.py; the gallery means are those
of golden_inpaint_game.npz, copied so that the tests read this file alone.

Stored per case <key>/...: seed; pg32 / pr32 (the reference as it is), pg64 / pr64 (the same network cast to .double()); r = max|d32 - d64| /
max|d64| over both distances; excluded (bool per level: |pg64 - pr64| <= 10 r max|d64|); cls64; first_on of the HARD masks (uint8 per map, the
generator asserts that they are nested and rebuild from it); iou_counts of the hard masks against the rectangle; with a blur: soft_levels (three
level indices), soft_rows (three row indices) and soft (maps x 3 levels x 3 rows x W float64, the reference's blurred masks there).

Conditions on every case (asserted; the next seed is tried where one fails):
  * percent-density: make_golden_inpaint_game's conditions (no cumulative value within 1e-10 of a threshold, no two positive keys equal);
  * cls[0] is false in both precisions;
  * at most 10 of 101 levels (3 of 32) are excluded."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)
import make_golden_inpaint_game as base  # noqa: E402  (loads the reference)
import inpaint_game_inputs as I  # noqa: E402
import inpaint_soft_inputs as J  # noqa: E402
from parity_utils import make_backbone  # noqa: E402

G, ns, ref_net, Double = base.G, base.ns, base.ref_net, base.Double


def run_case(out, name, wb32, wb64, gal_orig, gal_inp):
    arch, method, levels, include_zero, n_maps, blur = J.CASES[name]
    a, b = I.probe_pair(arch)
    gt = I.ground_truth(arch)
    L = len(levels)
    allowed = {101: 10, 32: 3}[L]
    for seed in range(200, 240):
        maps = J.maps_of(name, seed)
        why = None
        if method == 'percent-density':
            for m in maps:
                why = why or base.conditions(m, method, levels, seed, include_zero)
        res = []
        for m in maps if why is None else []:
            assert m.dtype == np.float64
            kw = dict(include_zero_elements=include_zero, mask_blur_sigma=blur, percentiles=levels, seed=seed)
            try:
                c32, pg32, pr32, blends, masks = G.classified_as_inpainted_twin(wb32, a, b, gal_orig, gal_inp, m, method, return_transitions=True, **kw)
                c64, pg64, pr64 = G.classified_as_inpainted_twin(Double(wb64), a, b, gal_orig.astype(np.float64), gal_inp.astype(np.float64), m, method, **kw)
            except AssertionError:
                why = 'cls[0] is true'
                break
            hard = G.create_threshold_masks(m, method, percentiles=levels, seed=seed, include_zero_elements=include_zero)
            assert hard.dtype == bool and (hard[1:] >= hard[:-1]).all(), 'the masks are not nested'
            first_on = (L - hard.sum(axis=0)).astype(np.uint8)
            assert np.array_equal(first_on[None] <= np.arange(L)[:, None, None], hard)
            if blur is None:
                assert np.array_equal(masks, hard)
                soft = None
            else:
                assert masks.dtype == np.float64 and np.array_equal(masks[levels == 100], hard[levels == 100].astype(np.float64))
                assert np.array_equal(blends, (1.0 - masks[:, None]) * a.astype(np.float64)[None] + masks[:, None] * b.astype(np.float64)[None])
                soft = masks[J.stored_levels(L)][:, J.stored_rows(m.shape[0])]
            counts = np.stack([(gt[None] & hard).sum(axis=(1, 2)), (gt[None] | hard).sum(axis=(1, 2)), (~gt[None] & hard).sum(axis=(1, 2))], axis=1)
            top = max(np.abs(pg64).max(), np.abs(pr64).max())
            r = max(np.abs(pg32 - pg64).max(), np.abs(pr32 - pr64).max()) / top
            excluded = np.abs(pg64 - pr64) <= 10 * r * top
            if excluded.sum() > allowed:
                why = '%d levels hinge on rounding' % excluded.sum()
                break
            assert np.array_equal(c64[~excluded], c32[~excluded])
            res.append((first_on, counts.astype(np.int64), pg32, pr32, pg64, pr64, r, excluded, c64, soft))
        print('  %-20s seed %d  %s' % (name, seed, why or 'ok  r = %s  excluded %s  twin from level %s' % (
            ['%.2e' % x[6] for x in res], [int(x[7].sum()) for x in res], [int(np.argmax(x[8])) for x in res])), flush=True)
        if why is None:
            break
    else:
        raise RuntimeError('%s: no seed meets the conditions' % name)
    out[name + '/seed'] = np.int64(seed)
    out[name + '/first_on'] = np.stack([x[0] for x in res])
    out[name + '/iou_counts'] = np.stack([x[1] for x in res])
    for j, key in enumerate(('pg32', 'pr32', 'pg64', 'pr64')):
        out[name + '/' + key] = np.stack([np.asarray(x[2 + j], dtype=np.float64) for x in res])
    out[name + '/r'] = np.float64(max(x[6] for x in res))
    out[name + '/excluded'] = np.stack([x[7] for x in res])
    out[name + '/cls64'] = np.stack([x[8] for x in res])
    if blur is not None:
        out[name + '/soft_levels'] = J.stored_levels(L)
        out[name + '/soft_rows'] = J.stored_rows(maps.shape[1])
        out[name + '/soft'] = np.stack([x[9] for x in res])


def main():
    game = np.load(os.path.join(HERE, 'golden_inpaint_game.npz'))
    out, nets = {}, {}
    only = sys.argv[1:]
    for name, case in J.CASES.items():
        arch = case[0]
        if only and name not in only:
            continue
        t = time.time()
        key = name.split('/')[0]
        if arch not in nets:
            ncls = I.NUM_CLASSES[arch]
            bb, sd = make_backbone(arch, seed=0, num_classes=ncls)
            wb32 = ns.whitebox.Whitebox(ref_net(arch, sd, ncls))
            wbn64 = ref_net(arch, sd, ncls)
            wbn64.net.double()
            nets[arch] = (wb32, ns.whitebox.Whitebox(wbn64), game[key + '/gal_orig'], game[key + '/gal_inp'])
            out[key + '/gal_orig'], out[key + '/gal_inp'] = nets[arch][2], nets[arch][3]
        run_case(out, name, *nets[arch])
        print('  %-20s %.1fs' % (name, time.time() - t), flush=True)
    if only:
        return print('cases named on the command line: a dry run, nothing is written')
    path = os.path.join(HERE, 'golden_inpaint_soft.npz')
    np.savez_compressed(path, **out)
    print('done: %s, %.0f KB' % (path, os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
