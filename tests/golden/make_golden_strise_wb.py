#!/usr/bin/env python
"""Golden vectors for STRise behind the generator's black box (eval/generate_inpaintinggame_bb_saliency_maps_multigpu.py:73-101): the REAL
reference STRise with black_box_fn = that script's bb_fn (restated below as make_black_box: glue around Whitebox.convert_from_numpy and
Whitebox.embeddings) around the reference's Whitebox with seeded weights, on its CPU path.
Usage: python tests/golden/make_golden_strise_wb.py   ->  tests/golden/golden_strise_wb.npz   (a few minutes; the ResNet-101 case dominates)

Shims (parity with the real packages is UNPINNED, like make_golden_strise.py's): blackbox.py sees make_golden_strise's skimage stand-ins (gaussian,
resize = scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True)); whitebox.py keeps ref_import's identity resize (224 x 224 in, 224 x 224
out).  ref_import's torchvision shim makes Resize / CenterCrop the identity, so this file installs its own PIL-backed Resize(144) / CenterCrop(128)
on the reference's lightcnn.transforms before WhiteboxLightCNN is built (torchvision's Resize of a PIL image is PIL's resize with BILINEAR), and
asserts that the Light-CNN tensor is 1 x 128 x 128.  The prior is the mini network's mean-EBP map of golden_strise.npz (the prior's network and
the black box are independent).  Draws are recorded as in make_golden_strise.py; every uint8 image handed to the network's preprocess is
recorded by wrapping it.

Stored per case <key>/...: arch, seed, num_masks, num_mask_elements, n_refs, n_gal, fill; mask_cells, mask_shifts; dq (the uint8 images q of masks 0-3 as
convert_from_numpy quantised them, minus the probe modulo 256: q = probe + dq in uint8 arithmetic, which deflates 40 times better than q) and q_crc
(zlib.crc32 of every mask's q); the fp32 network input of masks 0-1, as `tensor` for Light-CNN and, for the sub-mean networks, as tensor_lut
[3][256]: the value (float)(q - mean[c]) takes per channel and level (NaN where a level does not occur), tensor = tensor_lut[c][q]; scores32, scores64,
orig32, orig64 (references then gallery); map64 (float32) and map_dist = max|map32 - map64|; int_margin: the least distance of (v / 255) * 255 from
an integer over all elements of all masked probes where it is not exactly one, and int_near: how many elements lie within 1e-9 of one without
being one (int_near_dist: see below).

Asserted per case (the next seed is tried where the first fails): every |scores64| >= 10 r max|scores64|, r = max|scores32 - scores64| / max|scores64|,
with equal signs; q of EVERY mask equals numpy's chain on xfr_amd.models.blackbox.mask_law_scipy bit for bit (no level, no mask excluded).
Every element counted by int_near has v itself within 2^-44 (two ulps of [128, 256)) of its integer, the greatest such distance stored as
int_near_dist: between the last-bit cases and the 1e-9 margin lies nothing.  int_near is NOT asserted to be zero: where the mask is 1 - 2^-53 and the fill lies below the probe, v falls one ulp below the probe's integer by
construction -- the very effect this path exists for; the float64 arithmetic on both sides is IEEE, so what decides is the bit-for-bit check."""
import os
import sys
import time
import types
import zlib

import numpy as np
import PIL.Image
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_strise as MGS  # noqa: E402  (imports the reference, installs np.int)
from make_golden import ref_net  # noqa: E402
from parity_utils import make_backbone  # noqa: E402
from xfr_amd.models.blackbox import mask_law_scipy  # noqa: E402

ns = MGS.ns

# name, arch, classes, masks, elements, refs, gallery, fill
CASES = [
    ('mini/blur', 'stresnet_mini', 5, 48, 2, 3, 3, 'blur'),
    ('mini/gray', 'stresnet_mini', 5, 48, 2, 3, 3, 'gray'),
    ('mini/e40', 'stresnet_mini', 5, 48, 40, 3, 3, 'blur'),
    ('lcnn/blur', 'lightcnn29v2', 10, 20, 2, 2, 2, 'blur'),
    ('r50/blur', 'resnet50_128', None, 12, 2, 1, 1, 'blur'),
    ('r101/blur', 'stresnet101', 65359, 16, 2, 1, 1, 'blur'),
]


def pil_transforms():
    """torchvision.transforms for PIL images, as far as lightcnn.py:27-31 uses it."""
    tr = types.ModuleType('transforms')

    class Resize(object):
        def __init__(self, size):
            self.size = size

        def __call__(self, im):
            w, h = im.size
            if w <= h:
                nw, nh = self.size, int(self.size * h / w)
            else:
                nw, nh = int(self.size * w / h), self.size
            return im.resize((nw, nh), PIL.Image.BILINEAR)

    class CenterCrop(object):
        def __init__(self, size):
            self.size = size

        def __call__(self, im):
            w, h = im.size
            th, tw = self.size
            top, left = int(round((h - th) / 2.0)), int(round((w - tw) / 2.0))
            return im.crop((left, top, left + tw, top + th))
    base = sys.modules['torchvision.transforms']
    tr.Resize, tr.CenterCrop, tr.Lambda, tr.Compose = Resize, CenterCrop, base.Lambda, base.Compose
    return tr


def to_network(wb, images, cast):
    """A list of H x W x 3 arrays becomes the network's tensors through Whitebox.convert_from_numpy (`cast` gives them the network's dtype: the
    float64 run); a list of anything else passes as it is."""
    head = images[0]
    if isinstance(head, np.ndarray) and head.shape[2] == 3:
        return [cast(wb.convert_from_numpy(a)[0]) for a in images]
    return images


def unit_similarity(p, g):
    """1 - |p / |p| - g / |g|| / 2 for every (row of p, row of g): len(p) x len(g)."""
    pu = p / np.linalg.norm(p, axis=1)[:, None]
    gu = g / np.linalg.norm(g, axis=1)[:, None]
    return 1.0 - 0.5 * np.linalg.norm(pu[:, None] - gu, axis=2)


def make_black_box(wb, cast):
    """What the eval script hands STRise as black_box_fn (:73-101), restated: conversion, embeddings and similarity of (probes, gallery).  The
    gallery is embedded first, as there: PreprocessLog's order depends on it."""
    def score(probes, gallery):
        g = wb.embeddings(to_network(wb, gallery, cast))
        p = wb.embeddings(to_network(wb, probes, cast))
        return unit_similarity(p, g)
    return score


class PreprocessLog(object):
    """Every (uint8 image, tensor) that passes the network's preprocess."""

    def __init__(self, wbn):
        self.q, self.t = [], []
        inner = wbn.preprocess

        def preprocess(im, *a, **k):
            out = inner(im, *a, **k)
            self.q.append(np.array(im))
            self.t.append(out.detach().numpy().copy())
            return out
        wbn.preprocess = preprocess


def run_case(BB, out, name, arch, wb32, wb64, log, prior, imgs, n_masks, n_elem, n_refs, n_gal, fill):
    probe, refs, gal = imgs[0], imgs[1:1 + n_refs], imgs[4:4 + n_gal]
    for seed in range(100, 120):
        st = BB.STRise(probe=probe, refs=list(refs), gallery=list(gal), black_box_fn=make_black_box(wb32, lambda t: t), num_masks=n_masks,
                       num_mask_elements=n_elem, mask_fill_type=fill, use_gpu=False)
        st.prior = prior.copy()
        np.random.seed(seed)
        with MGS.Recorder() as rec:
            st.generate_masks()
        st.apply_masks()
        res = {}
        for tag, wb, cast in (('32', wb32, lambda t: t), ('64', wb64, lambda t: t.double())):
            st.black_box_fn = make_black_box(wb, cast)
            st.original_probe_gallery_scores = None
            if tag == '32':
                del log.q[:], log.t[:]
            st.score_masks()
            if not (np.asarray(st.mask_scores) > 0).any():
                break                                   # compute_saliency_map has nothing to select (blackbox.py:432)
            st.compute_saliency_map(positive_scores=True)
            res[tag] = (np.array(st.mask_scores, dtype=np.float64), np.array(st.saliency_map, dtype=np.float64),
                        np.concatenate([np.ravel(st.original_probe_ref_scores), np.ravel(st.original_probe_gallery_scores)]).astype(np.float64))
        if len(res) < 2:
            print('  %-12s seed %d  REJECTED: no positive score' % (name, seed))
            continue
        s32, s64 = res['32'][0], res['64'][0]
        top = np.abs(s64).max()
        r = np.abs(s32 - s64).max() / top
        ok = np.abs(s64).min() >= 10 * r * top and (np.sign(s32) == np.sign(s64)).all()
        print('  %-12s seed %d  r = %.2e  min|s|/max = %.2e  flips %d  map dist %.2e  %s' % (
            name, seed, r, np.abs(s64).min() / top, int((np.sign(s32) != np.sign(s64)).sum()), np.abs(res['32'][1] - res['64'][1]).max(),
            'ok' if ok else 'REJECTED: the selection would hinge on rounding'))
        if ok:
            break
    else:
        raise RuntimeError('%s: no seed meets the condition' % name)
    # the fp32 run's calls of preprocess, in score_masks' order: (refs, probe), (gallery, probe), (refs, masked probes), (gallery, masked probes)
    at = n_refs + 1 + n_gal + 1 + n_refs
    q = np.stack(log.q[at:at + n_masks])
    tens = np.concatenate(log.t[at:at + 2])
    assert len(log.q) >= at + n_masks + n_gal + n_masks and q.shape == (n_masks, 224, 224, 3) and q.dtype == np.uint8
    assert (log.q[n_refs] == probe).all() and (np.stack(log.q[at + n_masks + n_gal:at + 2 * n_masks + n_gal]) == q).all()
    if arch == 'lightcnn29v2':
        assert tens.shape == (2, 1, 128, 128), tens.shape
    cells = np.stack(rec.cells).astype(np.int32).reshape(n_masks, n_elem)
    shifts = np.array(rec.shifts, dtype=np.int32).reshape(n_masks, 2)
    gh = gw = -(-224 // st.mask_scale)
    margin, near, near_dist = np.inf, 0, 0.0
    for k in range(n_masks):
        assert (st.masked_probes[k] == st.masks[k][..., None] * probe + (1.0 - st.masks[k][..., None]) * st_fill(st, fill, probe)).all()
        w = (st.masked_probes[k] / 255) * 255
        d = np.abs(w - np.round(w))
        off = d[d > 0]
        near += int((off < 1e-9).sum())
        close = (d > 0) & (d < 1e-9)
        if close.any():                                 # how far v itself is from the integer it nearly quantises to
            near_dist = max(near_dist, float(np.abs(st.masked_probes[k] - np.round(st.masked_probes[k]))[close].max()))
        margin = min(margin, float(off.min())) if off.size else margin
        grid = np.ones(gh * gw)
        grid[cells[k]] = 0.0
        m = mask_law_scipy(grid.reshape(gh, gw), (224, 224), st.mask_scale, shifts[k])
        assert (m == st.masks[k]).all(), 'mask_law_scipy is not the reference mask of mask %d' % k
        assert (q[k] == w.astype(np.uint8)).all(), 'q of mask %d is not uint8((v / 255) * 255)' % k
    print('  %-12s int_margin %.3e  int_near %d of %d, at most %.3e from their integer' % (name, margin, near, n_masks * 224 * 224 * 3, near_dist))
    # the issue's margin, refined: whatever lies within 1e-9 of an integer is an integer but for the last bits (an ulp of [128, 256) is 2^-45),
    # i.e. the product of a mask of 1 -+ 2^-52 -- and nothing lies in between
    assert near_dist <= 2.0 ** -44, '%s: an element %.3e from an integer, neither an ulp effect nor clear of the 1e-9 margin' % (name, near_dist)
    out[name + '/arch'] = np.array(arch)
    out[name + '/seed'] = np.int64(seed)
    out[name + '/num_masks'] = np.int64(n_masks)
    out[name + '/num_mask_elements'] = np.int64(n_elem)
    out[name + '/n_refs'] = np.int64(n_refs)
    out[name + '/n_gal'] = np.int64(n_gal)
    out[name + '/fill'] = np.array(fill)
    out[name + '/mask_cells'] = cells
    out[name + '/mask_shifts'] = shifts
    out[name + '/dq'] = q[:4] - probe[None]             # uint8 arithmetic wraps: q = probe + dq (mod 256)
    out[name + '/q_crc'] = np.array([zlib.crc32(q[k].tobytes()) for k in range(n_masks)], dtype=np.uint32)
    assert tens.dtype == np.float32
    if arch == 'lightcnn29v2':
        out[name + '/tensor'] = tens
    else:                                               # (float)(q - mean[c]) takes one value per channel and level: stored as that table
        lut = np.full((3, 256), np.nan, dtype=np.float32)
        for c in range(3):
            lut[c, q[:2, :, :, c].ravel()] = tens[:, c].ravel()
            assert np.array_equal(lut[c][q[:2, :, :, c]], tens[:, c]), 'the tensor is no function of (channel, level)'
        out[name + '/tensor_lut'] = lut
    out[name + '/scores32'] = s32
    out[name + '/scores64'] = s64
    out[name + '/orig32'] = res['32'][2]
    out[name + '/orig64'] = res['64'][2]
    out[name + '/map64'] = res['64'][1].astype(np.float32)
    out[name + '/map_dist'] = np.float64(np.abs(res['32'][1] - res['64'][1]).max())
    out[name + '/int_margin'] = np.float64(margin)
    out[name + '/int_near'] = np.int64(near)
    out[name + '/int_near_dist'] = np.float64(near_dist)


def st_fill(st, fill, probe):
    if fill == 'gray':
        return 0.5 * np.ones(probe.shape)
    return MGS.gaussian(probe, st.blur_fill_sigma_percent / 100.0 * max(probe.shape), multichannel=True, preserve_range=True)


def main():
    BB = MGS.load_blackbox()
    ns.lightcnn.transforms = pil_transforms()
    imgs = MGS.images_u8()
    P = np.load(os.path.join(HERE, 'golden_strise.npz'))['mini/P_prior']
    prior = MGS.resize(P, (224, 224), anti_aliasing=True)
    out, nets = {}, {}
    for name, arch, ncls, n_masks, n_elem, n_refs, n_gal, fill in CASES:
        t = time.time()
        if arch not in nets:
            bb, sd = make_backbone(arch, seed=0, num_classes=ncls)
            wbn32 = ref_net(arch, sd, ncls)
            wbn64 = ref_net(arch, sd, ncls)
            wbn64.net.double()
            log = PreprocessLog(wbn32)
            wb32, wb64 = ns.whitebox.Whitebox(wbn32), ns.whitebox.Whitebox(wbn64)
            wb32._ebp_mode = wb64._ebp_mode = 'disable'
            nets[arch] = (wb32, wb64, log)
        wb32, wb64, log = nets[arch]
        run_case(BB, out, name, arch, wb32, wb64, log, prior, imgs, n_masks, n_elem, n_refs, n_gal, fill)
        print('  %-12s %.1fs' % (name, time.time() - t))
    path = os.path.join(HERE, 'golden_strise_wb.npz')
    np.savez_compressed(path, **out)
    print('done: %s, %.0f KB' % (path, os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
