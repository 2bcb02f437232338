"""The inpainting game's scoring, with the reference's names and signatures (python/xfr/inpainting_game/inpainting_game.py:12-215), so that its
callers (eval/run_inpainting_game_eval.py:123-124, plot_inpainting_game.py:130-134) can import them from here unchanged:

    create_threshold_masks(saliency_map, threshold_method, percentiles, thresholds, seed, max_noise, include_zero_elements, blur_sigma)    :12-77
    classified_as_inpainted_twin(snet, original_imT, inpaint_imT, original_gal_embed, inpaint_gal_embed, saliency_map, ...)               :80-146
    intersect_over_union_thresholded_saliency(saliency_map, ground_truth, mask_threshold_method, ...)                                     :149-197
    ratio_mate_nonmate_saliency(saliency_mask, probe_mate_region, of_total)                                                               :200-215

create_threshold_masks is a complete host restatement (numpy): 'percent-density', 'percent-pixels' (any other method name without thresholds),
explicit thresholds, and blur_sigma, with skimage.filters.gaussian stated as scipy.ndimage.gaussian_filter(mode='nearest', truncate=4.0).

classified_as_inpainted_twin runs on the device (xfr_inpaint_score[_ex]: masks, hybrids, forward, distances, nothing crosses the bus but the two
images, the map and the noise) when `snet` is an xfr_amd Whitebox, the images are in network format at the engine's input size, and the method is
  * 'percent-density' with sorted percentiles, or explicit non-increasing thresholds;
  * 'percent-pixels' (any other method name without thresholds) with sorted percentiles: the host computes v, total = v.sum() and
    np.percentile(v / total, 100 - percentiles) with the two end overrides of :59-62, and passes them as explicit thresholds together with the
    total, so that the device divides by numpy's sum and compares the very values the percentiles were taken from;
  * any of these with a positive mask_blur_sigma, when the map is float64 (the reference blurs in the map's dtype, :69), percentiles are given and
    the radius int(4 sigma_px + 0.5), sigma_px = mask_blur_sigma * min(H, W) / 100, is at most 64: the masks are blurred on the device with
    gaussian_kernel1d's weights in scipy's summation order, percentile 100 left hard (:71-72), and the hybrids are the float64 blend.
Everything else -- unsorted levels, H x W x 3 images, a float32 map with a blur, a larger radius -- takes the host restatement through
snet.embeddings, as the reference does.  np.random.seed(seed); np.random.rand(H, W) stays on the host either way: the noise is the reference's,
uploaded once per call.

Additive: score_maps scores several maps of one probe in one native call (the `for method, suffix_aggr` loop of plot_inpainting_game.py:972 for
one probe), and intersect_over_union_thresholded_saliency takes an optional `snet` to count on the device (xfr_inpaint_iou).
"""
import numpy as np
import scipy.ndimage

FORCE_HOST = False      # True: every call takes the host restatement (parity tests compare the two paths)


def _noisy_normalised(saliency_map, seed, max_noise, include_zero_elements):
    """:26-41."""
    np.random.seed(seed)
    nonzero = 1 if include_zero_elements else (saliency_map != 0)
    s = saliency_map + nonzero * np.random.rand(*saliency_map.shape) * max_noise
    return s / s.sum()


def create_threshold_masks(saliency_map, threshold_method, percentiles=None, thresholds=None, seed=None, max_noise=1e-9,
                           include_zero_elements=True, blur_sigma=None):
    """n_levels x H x W masks, True where the hybrid shows the inpainted twin: everything above the level's threshold."""
    s = _noisy_normalised(saliency_map, seed, max_noise, include_zero_elements)
    if threshold_method == 'percent-density':
        order = np.argsort(s.flat)
        cdf = np.cumsum(s.flat[order])
        s.flat[order] = cdf
        s = s / s.max()
        thresholds = 1.0 - percentiles.astype(s.dtype) / 100
        if percentiles[-1] == 100:
            thresholds[-1] = 0
    elif thresholds is None:
        thresholds = np.percentile(s, 100 - percentiles)
        if percentiles[0] == 0:
            thresholds[0] = 1
        if percentiles[-1] == 100:
            thresholds[-1] = 0
    masks = s[np.newaxis, ...] > thresholds[:, np.newaxis, np.newaxis]
    if blur_sigma is not None and blur_sigma > 0:
        masks = masks.astype(saliency_map.dtype)
        for i in range(masks.shape[0]):
            if percentiles[i] == 100:
                continue
            masks[i] = scipy.ndimage.gaussian_filter(masks[i], blur_sigma * np.min(saliency_map.shape) / 100.0, mode='nearest', truncate=4.0)
    return masks


def gaussian_kernel1d(sigma, truncate=4.0):
    """The 2 r + 1 weights of scipy.ndimage.gaussian_filter(sigma, truncate), r = int(truncate * sigma + 0.5), bit for bit (its _gaussian_kernel1d
    of order 0): what xfr_inpaint_options.blur_kernel_host takes."""
    sigma = float(sigma)
    radius = int(truncate * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return w / w.sum()


def _is_native(snet):
    from .models.whitebox import Whitebox
    return isinstance(snet, Whitebox)


def _is_device_tensor(maps):
    import torch
    return isinstance(maps, torch.Tensor) and maps.is_cuda


def _device_levels(threshold_method, percentiles, thresholds):
    """(method name, levels) when the device implements the request, else None.  'percent-pixels' stands for any other method name without
    thresholds (:57): its levels are the percentiles, which _pixel_thresholds turns into explicit thresholds per map."""
    if threshold_method == 'percent-density' or thresholds is None:
        if percentiles is None:
            return None
        p = np.asarray(percentiles, dtype=np.float64).ravel()
        ok = 1 <= p.size <= 255 and np.all(np.diff(p) >= 0) and p.min() >= 0 and p.max() <= 100
        return ('percent-density' if threshold_method == 'percent-density' else 'percent-pixels', p) if ok else None
    t = np.asarray(thresholds, dtype=np.float64).ravel()
    ok = 1 <= t.size <= 255 and np.all(np.isfinite(t)) and np.all(np.diff(t) <= 0)
    return ('thresholds', t) if ok else None


def _pixel_thresholds(maps, percentiles, noise, max_noise, include_zero_elements):
    """:26-41 and :57-62 on the host for n_maps x H x W maps: -> (thresholds n_maps x n_levels, totals n_maps).  The device divides the same v by
    the same total, so it compares numpy's s with thresholds taken from numpy's s."""
    thr, totals = [], []
    for m in maps:
        nonzero = 1 if include_zero_elements else (m != 0)
        v = m + nonzero * noise * max_noise
        total = v.sum()
        t = np.percentile(v / total, 100 - percentiles)
        if percentiles[0] == 0:
            t[0] = 1
        if percentiles[-1] == 100:
            t[-1] = 0
        thr.append(t)
        totals.append(total)
    return np.asarray(thr, dtype=np.float64), np.asarray(totals, dtype=np.float64)


def _device_blur(mask_blur_sigma, shape, dtype, percentiles, n_levels):
    """None: no blur.  False: a blur the device does not implement.  Else (kernel, flags) for the engine's blur_kernel / blur_levels."""
    if mask_blur_sigma is None or not mask_blur_sigma > 0:
        return None
    if np.dtype(dtype) != np.float64 or percentiles is None or np.size(percentiles) != n_levels:
        return False
    from ._lib import INPAINT_MAX_BLUR_RADIUS
    kernel = gaussian_kernel1d(mask_blur_sigma * np.min(shape) / 100.0)
    if not 1 <= kernel.size // 2 <= INPAINT_MAX_BLUR_RADIUS:
        return False          # radius 0 is scipy's one-tap kernel [1.0]: a float64 copy, left to the host
    return kernel, np.asarray(percentiles).ravel() != 100


def _engine_request(levels, maps, noise, max_noise, include_zero_elements, blur):
    """The engine's (levels, keywords) of a request _device_levels accepted; blur is _device_blur's answer (not False)."""
    kw = dict(method=levels[0], noise=noise, max_noise=max_noise, include_zero=include_zero_elements)
    lv = levels[1]
    if levels[0] == 'percent-pixels':
        lv, totals = _pixel_thresholds(maps, levels[1], noise, max_noise, include_zero_elements)
        kw.update(method='thresholds', totals=totals, levels_per_map=True)
    if blur:
        kw.update(blur_kernel=blur[0], blur_levels=blur[1])
    return lv, kw


def _network_format(snet, *images):
    shape = tuple(snet._engine(snet.batch_size).program.in_shape)
    return all(tuple(np.shape(im)) == shape for im in images)


def score_maps(wb, orig_imT, inpaint_imT, gal_orig, gal_inp, maps, percentiles=None, thresholds=None, mask_threshold_method='percent-density',
               seed=None, max_noise=1e-9, include_zero_elements=True, mask_blur_sigma=None):
    """Additive: the game of several maps (n_maps x H x W) of one probe in one native call.
    -> (classified_as_twin bool, pg_dist float64, pr_dist float64), each n_maps x n_levels.
    `maps` may be a float64 device tensor (what Engine.finish_saliency returns): under 'percent-density' and explicit thresholds the engine reads it
    where it lies, without a host copy; 'percent-pixels' takes its thresholds from numpy's percentile of the map, so the tensor is copied to the
    host first, as a host array is used today."""
    levels = _device_levels(mask_threshold_method, percentiles, thresholds)
    if levels is None:
        raise ValueError('score_maps runs on the device: percent-density or percent-pixels with sorted percentiles in [0, 100], or non-increasing '
                         'explicit thresholds, at most 255 levels')
    on_device = _is_device_tensor(maps)
    if on_device and str(maps.dtype) != 'torch.float64':
        raise ValueError('score_maps takes a device tensor as float64 maps (Engine.finish_saliency returns them), got %s' % maps.dtype)
    if on_device and levels[0] == 'percent-pixels':
        maps, on_device = maps.cpu().numpy(), False
    blur = _device_blur(mask_blur_sigma, tuple(maps.shape)[-2:] if on_device else np.shape(maps)[-2:], np.float64 if on_device else np.asarray(maps).dtype,
                        percentiles, len(levels[1]))
    if blur is False:
        raise ValueError('score_maps blurs on the device: float64 maps, percentiles given, a radius int(4 sigma_px + 0.5) of 1 to 64')
    if not on_device:
        maps = np.asarray(maps, dtype=np.float64)
    if len(maps.shape) == 2:
        maps = maps[None]
    np.random.seed(seed)
    noise = np.random.rand(*maps.shape[1:])
    eng = wb._engine(wb.batch_size)
    lv, kw = _engine_request(levels, maps, noise, max_noise, include_zero_elements, blur)
    cls, pg, pr = eng.inpaint_score(maps, lv, orig_imT, inpaint_imT, np.asarray(gal_orig, dtype=np.float32), np.asarray(gal_inp, dtype=np.float32),
                                    wb.net._mark('encode'), **kw)
    return cls.cpu().numpy().astype(bool), pg.cpu().numpy(), pr.cpu().numpy()


def _takes_device_path(snet, original_imT, inpaint_imT, saliency_map, mask_threshold_method, mask_blur_sigma, percentiles, thresholds):
    """(levels, blur) when classified_as_inpainted_twin runs on the device, else None: the routing stated in the module docstring."""
    if FORCE_HOST or not _is_native(snet):
        return None
    levels = _device_levels(mask_threshold_method, percentiles, thresholds)
    if levels is None:
        return None
    if not _network_format(snet, original_imT, inpaint_imT) or tuple(np.shape(saliency_map)) != tuple(np.shape(original_imT))[1:]:
        return None
    if levels[0] == 'percent-pixels' and not (np.min(saliency_map) >= 0 and np.sum(saliency_map) > 0):
        return None          # thresholds that may rise with the level: the host's
    blur = _device_blur(mask_blur_sigma, np.shape(saliency_map), np.asarray(saliency_map).dtype, percentiles, len(levels[1]))
    return None if blur is False else (levels, blur)


def classified_as_inpainted_twin(snet, original_imT, inpaint_imT, original_gal_embed, inpaint_gal_embed, saliency_map, mask_threshold_method,
                                 include_zero_elements=True, mask_blur_sigma=None, percentiles=None, thresholds=None, seed=None,
                                 binary_classification=True, return_transitions=False):
    """Switches original_imT to inpaint_imT under the thresholded saliency map and reports, per level, whether the hybrid is nearer to the inpainted
    subject's gallery mean than to the original's.  -> (classified_as_twin, pg_dist, pr_dist[, blends, masks])."""
    native = _takes_device_path(snet, original_imT, inpaint_imT, saliency_map, mask_threshold_method, mask_blur_sigma, percentiles, thresholds)
    if native is not None:
        levels, blur = native
        cls, pg, pr = score_maps(snet, original_imT, inpaint_imT, original_gal_embed, inpaint_gal_embed, saliency_map, percentiles=percentiles,
                                 thresholds=thresholds, mask_threshold_method=mask_threshold_method, seed=seed,
                                 include_zero_elements=include_zero_elements, mask_blur_sigma=mask_blur_sigma if blur else None)
        classified_as_twin, pg_dist, pr_dist = cls[0], pg[0], pr[0]
        assert not classified_as_twin[0]
        if not return_transitions:
            return classified_as_twin, pg_dist, pr_dist
        np.random.seed(seed)
        sal = np.asarray(saliency_map, dtype=np.float64)[np.newaxis]
        lv, kw = _engine_request(levels, sal, np.random.rand(*np.shape(saliency_map)), 1e-9, include_zero_elements, blur)
        eng = snet._engine(snet.batch_size)
        a, b = np.asarray(original_imT, dtype=np.float64), np.asarray(inpaint_imT, dtype=np.float64)
        if blur:
            masks = eng.inpaint_soft_masks(sal, lv, **kw).cpu().numpy()
            rgb_masks = masks[:, np.newaxis]
            blends = (1.0 - rgb_masks) * a[np.newaxis] + rgb_masks * b[np.newaxis]
        else:
            first_on = eng.inpaint_masks(sal, lv, **kw).cpu().numpy()[0]
            masks = first_on[np.newaxis] <= np.arange(len(levels[1]))[:, np.newaxis, np.newaxis]
            blends = np.where(masks[:, np.newaxis], b[np.newaxis], a[np.newaxis])
        return classified_as_twin, pg_dist, pr_dist, blends, masks

    masks = create_threshold_masks(saliency_map, threshold_method=mask_threshold_method, percentiles=percentiles, thresholds=thresholds, seed=seed,
                                   include_zero_elements=include_zero_elements, blur_sigma=mask_blur_sigma)
    if original_imT.shape[0] == 1 or original_imT.shape[-1] != 3:
        rgb_masks = masks[:, np.newaxis, ...]
    elif original_imT.shape[0] == 3 or original_imT.shape[-1] != 3:
        rgb_masks = np.repeat(masks[:, np.newaxis, :, :], 3, axis=1)
    else:
        rgb_masks = np.repeat(masks[:, :, :, np.newaxis], 3, axis=-1)
    a, b = np.asarray(original_imT).astype(np.float64), np.asarray(inpaint_imT).astype(np.float64)
    if masks.dtype == bool:
        blends = np.where(rgb_masks, b[np.newaxis], a[np.newaxis])        # (1 - m) * a + m * b for 0/1 masks, bit for bit
    else:
        blends = (1.0 - rgb_masks) * a[np.newaxis] + rgb_masks * b[np.newaxis]
    blend_embeds = snet.embeddings(blends)
    blend_embeds = blend_embeds / np.linalg.norm(blend_embeds, axis=1, keepdims=True)
    pr_dist = np.linalg.norm(blend_embeds - original_gal_embed, axis=1)
    pg_dist = np.linalg.norm(blend_embeds - inpaint_gal_embed, axis=1)
    classified_as_twin = pg_dist < pr_dist
    assert not classified_as_twin[0]
    if return_transitions:
        return classified_as_twin, pg_dist, pr_dist, blends, masks
    return classified_as_twin, pg_dist, pr_dist


def iou_counts(saliency_map, ground_truth, mask_threshold_method, percentiles=None, thresholds=None, seed=None, include_zero_elements=True, snet=None):
    """Additive: n_levels x 3 integer counts |gt & mask|, |gt | mask|, |~gt & mask| (:178-192), on the device where `snet` is an xfr_amd Whitebox
    and the device implements the method, else on the host."""
    gt = np.asarray(ground_truth).astype(bool)
    levels = _device_levels(mask_threshold_method, percentiles, thresholds)
    if (not FORCE_HOST and snet is not None and levels is not None and _is_native(snet)
            and tuple(np.shape(saliency_map)) == tuple(snet._engine(1).program.in_shape)[1:]
            and (levels[0] != 'percent-pixels' or (np.min(saliency_map) >= 0 and np.sum(saliency_map) > 0))):
        np.random.seed(seed)
        sal = np.asarray(saliency_map, dtype=np.float64)[np.newaxis]
        lv, kw = _engine_request(levels, sal, np.random.rand(*np.shape(saliency_map)), 1e-9, include_zero_elements, None)
        return snet._engine(1).inpaint_iou(sal, lv, gt, **kw).cpu().numpy()[0]
    masks = create_threshold_masks(saliency_map, threshold_method=mask_threshold_method, percentiles=percentiles, thresholds=thresholds, seed=seed,
                                   include_zero_elements=include_zero_elements)
    return np.stack([(gt[np.newaxis] & masks).sum(axis=(1, 2)), (gt[np.newaxis] | masks).sum(axis=(1, 2)),
                     (np.invert(gt)[np.newaxis] & masks).sum(axis=(1, 2))], axis=1).astype(np.int64)


def intersect_over_union_thresholded_saliency(saliency_map, ground_truth, mask_threshold_method, percentiles=None, thresholds=None, seed=None,
                                              include_zero_elements=True, return_fpos=False, return_tpos=False, snet=None):
    """Intersection over union of the thresholded saliency map with the ground-truth region, per level; with return_fpos / return_tpos also the
    false-positive and true-positive pixel counts.  snet (additive): count on the device."""
    counts = iou_counts(saliency_map, ground_truth, mask_threshold_method, percentiles=percentiles, thresholds=thresholds, seed=seed,
                        include_zero_elements=include_zero_elements, snet=snet)
    ret = (counts[:, 0] / (counts[:, 1] + 1e-9),)
    if return_fpos:
        ret += (counts[:, 2],)
    if return_tpos:
        ret += (counts[:, 0],)
    return ret[0] if len(ret) == 1 else ret


def ratio_mate_nonmate_saliency(saliency_mask, probe_mate_region, of_total=True):
    """The shares of the saliency mask inside and outside the mated region: of the whole image (of_total) or of each region."""
    inside = np.nansum(saliency_mask * probe_mate_region)
    outside = np.nansum(saliency_mask * (1.0 - probe_mate_region))
    if of_total:
        inside /= probe_mate_region.size
        outside /= probe_mate_region.size
    else:
        inside /= np.nansum(probe_mate_region)
        outside /= np.nansum(1.0 - probe_mate_region)
    return (inside, outside)


__all__ = ['create_threshold_masks', 'classified_as_inpainted_twin', 'intersect_over_union_thresholded_saliency', 'ratio_mate_nonmate_saliency',
           'score_maps', 'iou_counts', 'gaussian_kernel1d']
