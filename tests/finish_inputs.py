"""What the host and the GPU tests of saliency finishing share (test_finish_inputs, test_gpu_finish): seeded maps and probes, the two truths, and the
numpy restatement of the closed form the kernels of xfr_amd/csrc/finish.hip evaluate.

Truth.  host_chain(m, probe) is xfr_amd.saliency_io's own functions in create_save_smap's order, unmodified.  host_chain_exact_total is the same with
the ONE stated substitution: the float32 `sum()` of the shifted map (numpy's pairwise float32 sum, a few ulp off) is replaced by
np.float32(math.fsum(...)), the float32 nearest to the exact sum -- what the device divides by when the caller passes no totals.
A constant map: create_save_smap divides 0 by 0 and stores NaN.  The device states the all-zero map instead (include/xfr_amd.h), whose overlay is the
image; constant_truth() is that statement through saliency_io's own processSaliency and blend_saliency_map.
"""
import functools
import math

import numpy as np
import scipy.ndimage as ndi

from xfr_amd import saliency_io as SIO

PAD = 12
POLE = math.sqrt(3.0) - 2.0

# name -> (map kind, (h, w), (H, W)): the smallest shapes at which each part can go wrong, and the generator's own
CASES = {
    'pad_only_1x1': ('field', (1, 1), (4, 4)),                  # lines that are all padding but one value; one pixel is a constant map
    'pad_only_1x2': ('field', (1, 2), (4, 5)),                  # ... and the smallest map that is not
    'tiny_2x2': ('field', (2, 2), (3, 5)),
    'odd_3x4': ('field', (3, 4), (9, 7)),                       # non-square, non-integer factors
    'double_7x5': ('field', (7, 5), (14, 10)),
    'blocks_16x16': ('field', (16, 16), (48, 40)),              # more than one workgroup of output pixels
    'generator': ('field', (112, 112), (224, 224)),
    'generator_nonsquare': ('field', (112, 112), (160, 224)),
    'identity_112': ('field', (112, 112), (112, 112)),
    'identity_224': ('field', (224, 224), (224, 224)),
    'constant': ('constant', (16, 16), (48, 40)),
    'one_pixel': ('one_pixel', (16, 16), (48, 40)),
}


def is_constant(name):
    return CASES[name][0] == 'constant' or CASES[name][1] == (1, 1)


VARYING = [k for k in CASES if not is_constant(k)]
BATCHES = (1, 3, 33)


def seeded_map(kind, shape, seed):
    """float32 h x w.  field: a smoothed random field to the fourth power, its lowest 30 % set to zero, sum 1 -- exact zeros and, resized, clipped
    undershoot, like a real EBP map."""
    rng = np.random.RandomState(1000 + seed)
    h, w = shape
    if kind == 'constant':
        return np.full(shape, 0.25, dtype=np.float32)
    if kind == 'one_pixel':
        m = np.zeros(shape, dtype=np.float32)
        m[rng.randint(h), rng.randint(w)] = 1.0
        return m
    f = ndi.gaussian_filter(rng.rand(h, w), sigma=max(1.0, min(h, w) / 16.0), mode='nearest') if min(h, w) > 1 else rng.rand(h, w)
    f = (f - f.min() + 0.05) ** 4
    if f.size > 3:
        f[f < np.percentile(f, 30)] = 0.0
    return (f / f.sum()).astype(np.float32)


def seeded_probe(shape, seed):
    """uint8 H x W x 3."""
    return np.random.RandomState(2000 + seed).randint(0, 256, tuple(shape) + (3,)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def batch(name, n):
    """(maps float32 n x h x w, probes uint8 n x H x W x 3) of a case; map i of every batch size is the same map."""
    kind, hw, HW = CASES[name]
    maps = np.stack([seeded_map(kind, hw, i) for i in range(n)])
    probes = np.stack([seeded_probe(HW, i) for i in range(n)])
    maps.setflags(write=False)
    probes.setflags(write=False)
    return maps, probes


def _head(m, exact_total):
    smap = np.asarray(m).astype(np.float32)                       # create_save_smap, saliency_io.py
    smap = smap - smap.min()
    total = np.float32(math.fsum(smap.ravel().tolist())) if exact_total else smap.sum()
    return smap / total, total


def _tail(smap, probe):
    img = probe.astype(np.float64) / 255.0
    smap = SIO.processSaliency(img, smap)
    overlay = SIO.blend_saliency_map(img, smap)
    return smap, (np.clip(overlay, 0, 1) * 255).astype(np.uint8)


def host_chain(m, probe):
    """-> (saliency_map float64 H x W, overlay uint8 H x W x 3): what create_save_smap stores."""
    return _tail(_head(m, False)[0], probe)


def host_chain_exact_total(m, probe):
    return _tail(_head(m, True)[0], probe)


def numpy_total(m):
    """The float32 sum create_save_smap divides by: what a caller passes as `totals`."""
    return _head(m, False)[1]


def constant_truth(probe):
    """The all-zero map through saliency_io's own tail: (zeros H x W, the image's bytes)."""
    return _tail(np.zeros(probe.shape[:2], dtype=np.float32), probe)


@functools.lru_cache(maxsize=None)
def truth(name, n, exact_total):
    """The chain of every map of batch(name, n): (smaps n x H x W, overlays n x H x W x 3), computed once."""
    maps, probes = batch(name, n)
    if is_constant(name):
        out = [constant_truth(p) for p in probes]
    else:
        out = [(host_chain_exact_total if exact_total else host_chain)(m, p) for m, p in zip(maps, probes)]
    s, o = np.stack([x[0] for x in out]), np.stack([x[1] for x in out])
    s.setflags(write=False)
    o.setflags(write=False)
    return s, o


@functools.lru_cache(maxsize=None)
def reference_r(n=3):
    """r: the largest distance between host_chain and host_chain_exact_total over the first n maps of every varying case -- how far the reference is
    from itself when its float32 sum is replaced by the exact one.  Computed, never hard-coded (3.9e-8 on 20 generator maps, 1.8e-8 here)."""
    return max(float(np.abs(truth(name, n, False)[0] - truth(name, n, True)[0]).max()) for name in VARYING)


def resize_input(name, seed=0):
    """A float64 h x w array in [0, 1] with exact zeros for the resize alone: every case has one, the constant ones included."""
    a = np.random.RandomState(3000 + seed).rand(*CASES[name][1])
    a[a < 0.3] = 0.0
    return a


def normalised(m, exact_total=False):
    """The float64 map the resize starts from (processSaliency's first two lines on create_save_smap's float32 head)."""
    a = np.asarray(_head(m, exact_total)[0], dtype=np.float64)
    a = a - a.min()
    return a / (a.max() + 1e-9)


# ---- the closed form ---------------------------------------------------------------------------------------------------------------------
def _prefilter(c):
    """B-spline coefficients of every line of c along axis 0, in place (c: L x anything, float64)."""
    z = POLE
    L = c.shape[0]
    c *= (1.0 - z) * (1.0 - 1.0 / z)
    zn = z ** (L - 1)
    s = c[0] + zn * c[L - 1]
    zi = z
    for i in range(1, L - 1):
        s = s + zi * (c[i] + zn * c[L - 1 - i])
        zi *= z
    c[0] = s / (1.0 - zn * zn)
    for i in range(1, L):
        c[i] += z * c[i - 1]
    c[L - 1] = (z * c[L - 2] + c[L - 1]) * z / (z * z - 1.0)
    for i in range(L - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return c


def _taps(dim, out):
    x = (np.arange(out) + 0.5) * (dim / out) - 0.5 + PAD
    f = np.floor(x)
    t = x - f
    wts = np.stack([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6])
    return f.astype(np.int64) - 1, wts


def spline_resize(a, out_shape):
    """scipy.ndimage.zoom(a, order=3, mode='grid-constant', cval=0, grid_mode=True) to out_shape (no axis shrinks), then _resize_cubic's clip."""
    a = np.asarray(a, dtype=np.float64)
    if a.shape == tuple(out_shape):
        return a.copy()
    c = np.pad(a, PAD)
    _prefilter(c)
    c = _prefilter(np.ascontiguousarray(c.T)).T
    (fy, wy), (fx, wx) = _taps(a.shape[0], out_shape[0]), _taps(a.shape[1], out_shape[1])
    out = np.zeros(out_shape)
    for i in range(4):
        row = np.zeros(out_shape)
        for j in range(4):
            row += wx[j][None, :] * c[(fy + i)[:, None], (fx + j)[None, :]]
        out += wy[i][:, None] * row
    return np.clip(out, min(a.min(), 0.0), max(a.max(), 0.0))


def table_step_pixels(v):
    """Pixels of a finished map v where the host's att * 256 lies within 1e-9 of a positive integer: a step of the colour table."""
    att = v - v.min()
    if att.max() <= 0:
        return np.zeros(v.shape, dtype=bool)
    x = att / att.max() * 256
    return (np.abs(x - np.rint(x)) <= 1e-9) & (np.rint(x) >= 1)


NOISE_FLOOR = 1e-12


def overlay_check(name, got, want, v):
    """The overlay conditions of one map against the host's bytes `want` of its finished map v: at most 0.1 % of its pixels differ, none by more
    than one level in any channel but at a step of the colour table (those count towards the 0.1 % all the same).
    -> (pixels that differ anywhere, the largest level distance outside table steps, pixels of the map), for printing.
    The zero step.  The byte is uint8(((1 - alpha) k / 255 + alpha c) * 255), truncated: k at alpha == 0, k - 1 at ANY alpha > 0 where c < k / 255.
    Where a map's true value is zero -- whole rows of a small map, the far field of a one-pixel map -- scipy leaves either the clip's exact zero or
    rounding residue of 1e-16 and less, and the reference itself differs there from its own restatement (which agrees with it to 8e-16): 6 of 63
    pixels on the 3 x 4 maps, 122 of 1920 on the one-pixel map (test_finish_inputs.py runs this function on the reference alone).  No
    implementation held to 1e-12 on the map can be held to those bytes, so the 0.1 % is counted over the pixels whose host value lies more than
    NOISE_FLOOR, the map's own bar, above the map's minimum; the one-level condition holds on every pixel."""
    d = np.abs(got.astype(np.int64) - want.astype(np.int64)).max(axis=-1)
    step = table_step_pixels(v)
    counted = (d > 0) & (v - v.min() > NOISE_FLOOR)
    differ, apart = int(counted.sum()), int(d[~step].max()) if (~step).any() else 0
    assert differ <= 1e-3 * d.size, '%s: %d of %d pixels differ' % (name, differ, d.size)
    assert apart <= 1, '%s: %d levels apart' % (name, apart)
    return int((d > 0).sum()), apart, d.size
