#!/usr/bin/env python
"""Golden vectors for inpainting-game scoring (python/xfr/inpainting_game/inpainting_game.py:12-197), produced by the REAL reference functions on
the CPU.  Usage: python tests/golden/make_golden_inpaint_game.py  ->  tests/golden/golden_inpaint_game.npz

The reference module is imported unchanged through ref_import.load() (skimage.filters.gaussian is that file's scipy restatement); `np.bool = bool`
is this file's own shim for :168, which predates numpy 1.24.  Inputs are tests/inpaint_game_inputs.py: seeded, so only results are stored.
Gallery means: the unit-norm mean of the reference's fp32 embeddings of three (original, twin) pairs.

Stored per case <key>/...: seed; first_on (uint8, per map: the first level at which a pixel is on, n_levels where never -- the generator asserts
that the reference's masks are nested and rebuild from it); iou_counts (int64 n_levels x 3 against the rectangle: |gt & m|, |gt | m|, |~gt & m|);
pg32 / pr32 (the reference as it is) and pg64 / pr64 (the same network cast to .double(), inputs rounded to fp32 as the reference does);
r = max|d32 - d64| / max|d64| over both distances; excluded (bool per level: |pg64 - pr64| <= 10 r max|d64|).  Per network: gal_orig, gal_inp.

Conditions on every case (asserted; the next seed is tried where one fails):
  * for every threshold t > 0 no reference cdf value lies within 1e-10 of t (more than 10 x the worst-case float64 summation bound
    50176 * 2**-53), except the maximum, which is exactly 1 at t = 1 -- so no float64 summation order can flip a mask;
  * no two positive keys are equal (the order of the cumulative sum is then unique up to the zeros, which add nothing);
  * cls[0] is false in both precisions;
  * at most 10 of 101 levels (3 of 32, 1 of 5) are excluded."""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402
from parity_utils import make_backbone  # noqa: E402
import inpaint_game_inputs as I  # noqa: E402

ns = ref_import.load()
from make_golden import ref_net  # noqa: E402
import xfr.inpainting_game.inpainting_game as G  # noqa: E402

torch.set_num_threads(int(os.environ.get('XFR_THREADS', '8')))
if not hasattr(np, 'bool'):
    np.bool = bool          # inpainting_game.py:168


class Double(object):
    """The reference's Whitebox on a .double() network: embeddings() rounds the float64 hybrids to fp32 as whitebox.py:762 does, then widens."""

    def __init__(self, wb):
        self.wb = wb

    def embeddings(self, images):
        return self.wb.embeddings([torch.from_numpy(im).float().double() for im in images])


def reference_values(s_map, method, levels, seed, include_zero):
    """The array the reference compares with its thresholds (:26-52), restated to check the fixture's conditions."""
    np.random.seed(seed)
    nz = 1 if include_zero else (s_map != 0)
    s = s_map + nz * np.random.rand(*s_map.shape) * 1e-9
    s = s / s.sum()
    keys = s.ravel().copy()
    if method != 'percent-density':
        return s, keys, np.asarray(levels, dtype=np.float64)
    order = np.argsort(s.flat)
    s.flat[order] = np.cumsum(s.flat[order])
    s = s / s.max()
    thr = 1.0 - levels.astype(np.float64) / 100
    if levels[-1] == 100:
        thr[-1] = 0
    return s, keys, thr


def conditions(s_map, method, levels, seed, include_zero):
    vals, keys, thr = reference_values(s_map, method, levels, seed, include_zero)
    pos = np.sort(keys[keys > 0])
    if (np.diff(pos) == 0).any():
        return 'two positive keys are equal'
    v = vals.ravel()
    for t in thr:
        if t <= 0:
            continue
        near = np.abs(v - t) <= 1e-10
        if t == 1.0 and method == 'percent-density':
            near &= v != v.max()
        if near.any():
            return 'a value lies within 1e-10 of the threshold %r' % t
    return None


def run_case(out, name, wb32, wb64, gal_orig, gal_inp):
    arch, method, levels, include_zero, n_maps = I.CASES[name]
    a, b = I.probe_pair(arch)
    gt = I.ground_truth(arch)
    L = len(levels)
    allowed = {101: 10, 32: 3, 5: 1}[L]
    kw = dict(percentiles=levels) if method == 'percent-density' else dict(thresholds=levels)
    ref_method = method if method == 'percent-density' else 'mass-threshold'
    for seed in range(200, 240):
        maps = I.maps_of(name, seed)
        assert all((m == 0).mean() >= 0.2 and m.min() >= 0 for m in maps)
        why = None
        for m in maps:
            why = why or conditions(m, method, levels, seed, include_zero)
        res = []
        for m in maps if why is None else []:
            c32, pg32, pr32, blends, masks = G.classified_as_inpainted_twin(wb32, a, b, gal_orig, gal_inp, m, ref_method, include_zero_elements=include_zero,
                                                                            seed=seed, return_transitions=True, **kw)
            try:
                c64, pg64, pr64 = G.classified_as_inpainted_twin(Double(wb64), a, b, gal_orig.astype(np.float64), gal_inp.astype(np.float64), m, ref_method,
                                                                 include_zero_elements=include_zero, seed=seed, **kw)
            except AssertionError:
                why = 'cls[0] is true in float64'
                break
            assert masks.dtype == bool and (masks[1:] >= masks[:-1]).all(), 'the masks are not nested'
            first_on = (L - masks.sum(axis=0)).astype(np.uint8)
            assert np.array_equal(first_on[None] <= np.arange(L)[:, None, None], masks)
            assert np.array_equal(blends.astype(np.float32), np.where(masks[:, None], b[None], a[None])), 'the blend is not the select'
            iou, fpos, tpos = G.intersect_over_union_thresholded_saliency(m, gt, ref_method, seed=seed, include_zero_elements=include_zero,
                                                                          return_fpos=True, return_tpos=True, **kw)
            union = (gt[None] | masks).sum(axis=(1, 2))
            assert np.array_equal(tpos, (gt[None] & masks).sum(axis=(1, 2))) and np.allclose(iou, tpos / (union + 1e-9), rtol=0, atol=0)
            top = max(np.abs(pg64).max(), np.abs(pr64).max())
            r = max(np.abs(pg32 - pg64).max(), np.abs(pr32 - pr64).max()) / top
            excluded = np.abs(pg64 - pr64) <= 10 * r * top
            if excluded.sum() > allowed:
                why = '%d levels hinge on rounding' % excluded.sum()
                break
            assert np.array_equal(c64[~excluded], c32[~excluded])
            res.append((first_on, np.stack([tpos, union, fpos], axis=1).astype(np.int64), pg32, pr32, pg64, pr64, r, excluded, c64))
        print('  %-16s seed %d  %s' % (name, seed, why or 'ok  r = %s  excluded %s  twin from level %s' % (
            ['%.2e' % x[6] for x in res], [int(x[7].sum()) for x in res], [int(np.argmax(x[8])) for x in res])))
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


def main():
    out, nets = {}, {}
    for name, (arch, _, _, _, _) in I.CASES.items():
        t = time.time()
        if arch not in nets:
            ncls = I.NUM_CLASSES[arch]
            bb, sd = make_backbone(arch, seed=0, num_classes=ncls)
            wb32 = ns.whitebox.Whitebox(ref_net(arch, sd, ncls))
            wbn64 = ref_net(arch, sd, ncls)
            wbn64.net.double()
            wb64 = ns.whitebox.Whitebox(wbn64)
            pairs = I.gallery_pairs(arch)
            gal = []
            for side in (0, 1):
                e = wb32.embeddings([p[side] for p in pairs])
                e = e.reshape(len(pairs), -1).astype(np.float64).mean(axis=0)
                gal.append((e / np.linalg.norm(e)).astype(np.float32))
            nets[arch] = (wb32, wb64, gal[0], gal[1])
            out[name.split('/')[0] + '/gal_orig'] = gal[0]
            out[name.split('/')[0] + '/gal_inp'] = gal[1]
        run_case(out, name, *nets[arch])
        print('  %-16s %.1fs' % (name, time.time() - t))
    path = os.path.join(HERE, 'golden_inpaint_game.npz')
    np.savez_compressed(path, **out)
    print('done: %s, %.0f KB' % (path, os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
