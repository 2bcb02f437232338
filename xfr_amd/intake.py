"""Image intake: from decoded uint8 crops to the network-size uint8 batch of `Engine.forward_u8`, on the device (xfr_intake_u8[_host],
csrc/intake.hip) -- the arithmetic of `Whitebox.convert_from_numpy` (python/xfr/models/whitebox.py:787-806) behind `image_loader`
(python/xfr/utils.py:39-202): the / 255 head, `saliency_io.resize_linear` (a Gaussian pre-filter on the shrinking axes, scipy's order-1 mirror
zoom, the clip to the crop's range) and the truncation to bytes.

`host_bytes` is the numpy statement of that chain with no scipy in it: the law the kernels restate, equal to resize_linear + truncation byte for
byte (tests/test_intake_inputs.py).  Every operation is one rounded float64 operation in the order written; the truncation reads the last bit.
`pack` lays crops out as one source buffer with its item table, `device_bytes` runs them through the engine, `refusal` says which crops the
device call would refuse (those stay on the host)."""
import ctypes

import numpy as np

from . import _lib

HEAD_F64, HEAD_F32 = 0, 1      # XFR_INTAKE_HEAD_F64 (files, DataFrame rows: u / 255.0), XFR_INTAKE_HEAD_F32 (uint8 arrays: float32(u) / 255)
MAX_DIM, MAX_RADIUS = _lib.INTAKE_MAX_DIM, _lib.INTAKE_MAX_RADIUS


class IntakeRefused(ValueError):
    """The device path does not take these images (float arrays, a size the zoom rounds away from, ...): the host chain does."""


def head(u8, kind):
    """The / 255 of the chain as float64: exact float64 quotients (HEAD_F64) or float32 quotients widened (HEAD_F32)."""
    u8 = np.asarray(u8)
    if kind == HEAD_F32:
        return (u8.astype(np.float32) / np.float32(255)).astype(np.float64)
    return u8.astype(np.float64) / 255.0


def prefilter_of(n_in, n_out):
    """(sigma, radius) of the Gaussian pre-filter along an axis of n_in values resized to n_out; radius 0: no pass."""
    f = np.float64(n_in) / np.float64(n_out)
    if not f > 1:
        return 0.0, 0
    sigma = float((f - 1) / 2)
    if not sigma > 1e-15:
        return 0.0, 0
    return sigma, int(4.0 * sigma + 0.5)


def gaussian_weights(sigma, radius):
    """scipy.ndimage's _gaussian_kernel1d(sigma, 0, radius): 2 radius + 1 weights, numpy's exp and numpy's sum."""
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def fold_mirror(i, n):
    """Indices of a line of n values extended by mirroring without repeating the edge (period 2 (n - 1)); a line of one value is constant."""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def gaussian_axis(a, axis, sigma, radius):
    """scipy.ndimage.gaussian_filter1d(a, sigma, axis, mode='mirror') by hand: the centre term, then the pairs from the outermost inwards."""
    w = gaussian_weights(sigma, radius)
    a = np.moveaxis(a, axis, 0)
    n = a.shape[0]
    l = np.arange(n)
    out = a * w[radius]
    for ii in range(-radius, 0):
        out = out + (a[fold_mirror(l + ii, n)] + a[fold_mirror(l - ii, n)]) * w[radius + ii]
    return np.moveaxis(out, 0, axis)


def prefilter(a, out_hw):
    """The Gaussian pre-filter of resize_linear on a float64 h x w [x C] array: axis 0, then axis 1, each only where it shrinks."""
    for axis in (0, 1):
        sigma, radius = prefilter_of(a.shape[axis], out_hw[axis])
        if sigma > 0:
            a = gaussian_axis(a, axis, sigma, radius)
    return a


def zoom_taps(n, m):
    """(i0, i1, w0, w1) of scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True) along an axis of n values resized to m."""
    o = np.arange(m, dtype=np.float64)
    cc = (o + 0.5) * (np.float64(n) / np.float64(m)) - 0.5
    c = np.where(cc < 0, -cc, cc)
    if n == 1:
        c = np.zeros(m)
    st = np.floor(c)
    w0 = 1.0 - (c - st)
    w1 = 1.0 - w0
    i0 = st.astype(np.int64)
    return i0, fold_mirror(i0 + 1, n), w0, w1


def zoom_keeps_size(n, m):
    """scipy's zoom sizes its own output: round(n * zoom) with zoom = 1 / (n / m).  resize_linear pads or crops when that is not m."""
    return int(round(n * (1.0 / (np.float64(n) / np.float64(m))))) == m


def zoom_linear(a, out_hw):
    """The order-1 zoom of a float64 h x w x C array to H x W x C: the four products added in scipy's order."""
    y0, y1, wy0, wy1 = zoom_taps(a.shape[0], out_hw[0])
    x0, x1, wx0, wx1 = zoom_taps(a.shape[1], out_hw[1])
    wy0, wy1 = wy0[:, None, None], wy1[:, None, None]
    wx0, wx1 = wx0[None, :, None], wx1[None, :, None]
    t = 0.0 + (a[y0][:, x0] * wy0) * wx0
    t = t + (a[y0][:, x1] * wy0) * wx1
    t = t + (a[y1][:, x0] * wy1) * wx0
    return t + (a[y1][:, x1] * wy1) * wx1


def refusal(shape, out_hw):
    """Why the device call refuses a crop of `shape` (h, w [, C]) for an output of out_hw, or None: the argument checks of xfr_intake_u8."""
    h, w = int(shape[0]), int(shape[1])
    c = int(shape[2]) if len(shape) > 2 else 1
    H, W = int(out_hw[0]), int(out_hw[1])
    if c not in (1, 3, 4):
        return '%d channels' % c
    if not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM):
        return 'a crop of %d x %d' % (h, w)
    if (h, w) == (H, W):
        return None
    if max(prefilter_of(h, H)[1], prefilter_of(w, W)[1]) > MAX_RADIUS:
        return 'a pre-filter radius above %d' % MAX_RADIUS
    if not (zoom_keeps_size(h, H) and zoom_keeps_size(w, W)):
        return '%d x %d to %d x %d is a size the zoom rounds away from' % (h, w, H, W)
    return None


def host_bytes(u8_crop, out_hw, head_kind):
    """uint8 h x w [x C] crop, C in {1, 3, 4} -> the uint8 H x W x 3 image convert_from_numpy hands to the network's `preprocess`."""
    u = np.asarray(u8_crop)
    if u.dtype != np.uint8 or u.ndim not in (2, 3):
        raise ValueError('host_bytes takes a uint8 h x w [x C] crop, got %s of %s' % (u.dtype, u.shape))
    if u.ndim == 2:
        u = u[:, :, None]
    out_hw = (int(out_hw[0]), int(out_hw[1]))
    why = refusal(u.shape, out_hw)
    if why is not None:
        raise IntakeRefused('host_bytes: ' + why)
    if u.shape[:2] == out_hw:
        if head_kind == HEAD_F32:
            b = ((u.astype(np.float32) / np.float32(255)) * np.float32(255)).astype(np.uint8)
        else:
            b = (head(u, HEAD_F64) * 255.0).astype(np.uint8)
    else:
        a = head(u, head_kind)
        lo, hi = a.min(), a.max()
        v = zoom_linear(prefilter(a, out_hw), out_hw)
        b = (np.minimum(np.maximum(v, lo), hi) * 255.0).astype(np.uint8)
    if b.shape[2] == 1:
        return np.repeat(b, 3, axis=2)
    return np.ascontiguousarray(b[:, :, :3])


class Item(ctypes.Structure):
    """xfr_intake_item: a crop inside the source buffer."""
    _fields_ = [('offset', ctypes.c_int64), ('h', ctypes.c_int32), ('w', ctypes.c_int32), ('row_stride', ctypes.c_int32),
                ('channels', ctypes.c_int32), ('head', ctypes.c_int32)]


def pack(items):
    """[(uint8 h x w [x C] crop, head), ...] -> (source: one uint8 array holding every crop, rows contiguous, (Item * n) table)."""
    table = (Item * len(items))()
    offsets, total = [], 0
    for k, (u, kind) in enumerate(items):
        if u.dtype != np.uint8 or u.ndim not in (2, 3):
            raise ValueError('pack takes uint8 h x w [x C] crops, got %s of %s' % (u.dtype, u.shape))
        c = u.shape[2] if u.ndim == 3 else 1
        table[k] = Item(total, u.shape[0], u.shape[1], u.shape[1] * c, c, int(kind))
        offsets.append(total)
        total += u.shape[0] * u.shape[1] * c
    src = np.empty(max(total, 1), dtype=np.uint8)
    for off, (u, _) in zip(offsets, items):
        src[off:off + u.size].reshape(u.shape)[...] = u
    return src, table


def stated_kernels(items, out_hw):
    """numpy's Gaussian kernels for the pre-filters the items need: (sigmas, radii, weights n x (MAX_RADIUS + 1)) for Engine.intake_set_kernels."""
    seen = {}
    for u, _ in items:
        for axis in (0, 1):
            sigma, radius = prefilter_of(u.shape[axis], out_hw[axis])
            if 0 < radius <= MAX_RADIUS and (sigma, radius) not in seen:
                row = np.zeros(MAX_RADIUS + 1)
                row[:radius + 1] = gaussian_weights(sigma, radius)[:radius + 1]
                seen[(sigma, radius)] = row
    keys = sorted(seen)
    return (np.array([k[0] for k in keys], dtype=np.float64), np.array([k[1] for k in keys], dtype=np.int32),
            np.array([seen[k] for k in keys], dtype=np.float64).reshape(len(keys), MAX_RADIUS + 1))


def device_bytes(engine, items, out_hw, tables=None):
    """[(uint8 crop, head), ...] -> uint8 device tensor n x H x W x 3 (n x final_h x final_w x 3 behind `tables`, the (row, column) pair of
    pil_bilinear_tables): one xfr_intake_u8_host call.  Raises IntakeRefused where the call would refuse an item."""
    out_hw = (int(out_hw[0]), int(out_hw[1]))
    for k, (u, _) in enumerate(items):
        why = refusal(u.shape, out_hw)
        if why is not None:
            raise IntakeRefused('item %d: %s' % (k, why))
    src, table = pack(items)
    engine.intake_set_kernels(*stated_kernels(items, out_hw))
    return engine.intake_u8(src, table, out_hw, tables=tables)


def host_chain_bytes(items, out_hw, tables=None):
    """The same batch on the host, as a uint8 numpy array: host_bytes per crop, then apply_pil_tables."""
    out = [host_bytes(u, out_hw, kind) for u, kind in items]
    if tables is not None:
        from .models.blackbox import apply_pil_tables
        out = [apply_pil_tables(b, tables[0], tables[1]) for b in out]
    return np.stack(out)
