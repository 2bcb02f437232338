"""Host-side tests (no GPU) of soft-edged masks and 'percent-pixels' levels in inpainting-game scoring: the additive C ABI (the _ex forms and
xfr_inpaint_options), the summation order the soft kernels implement, the percent-pixels host routing, and which argument sets take the device."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.ndimage

import inpaint_game_inputs as I
from xfr_amd import _lib
from xfr_amd import inpainting_score as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX_SYMBOLS = ('xfr_inpaint_score_ex', 'xfr_inpaint_iou_ex', 'xfr_inpaint_debug_masks_ex', 'xfr_inpaint_debug_blends_ex', 'xfr_inpaint_debug_soft_masks')
BLUR_SHAPES = [((7, 9), 3.0), ((37, 53), 0.3), ((37, 53), 1.48), ((128, 128), 5.12), ((224, 224), 8.96), ((224, 224), 2.24)]


def blur_in_the_kernels_order(mask, w):
    """include/xfr_amd.h, blur_radius: axis 0 then axis 1, edge-clamped, t = in[0] w[r]; for j = r .. 1: t += (in[-j] + in[+j]) w[r - j]."""
    r = len(w) // 2
    out = np.asarray(mask, dtype=np.float64)
    for axis in (0, 1):
        x = np.moveaxis(out, axis, 0)
        n = x.shape[0]
        at = lambda d: x[np.clip(np.arange(n) + d, 0, n - 1)]
        t = at(0) * w[r]
        for j in range(r, 0, -1):
            t = t + (at(-j) + at(j)) * w[r - j]
        out = np.moveaxis(t, 0, axis)
    return out


def test_ex_symbols_declared_bound_exported_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, 'include', 'xfr_amd.h')).read()
    declared = set(re.findall(r'xfr_status\s+XFR_EX\s+(xfr_inpaint_\w+)\s*\(', hdr))
    assert declared == set(EX_SYMBOLS)
    bound = [n for n, _, _ in _lib.SYMBOLS]
    lib = _lib.load()
    for name in EX_SYMBOLS:
        assert name in bound and hasattr(lib, name)
    assert '#define XFR_AMD_ABI_VERSION 7' in hdr and _lib.ABI_VERSION == 7 and lib.xfr_abi_version() == 7
    assert '#define XFR_INPAINT_MAX_BLUR_RADIUS 64' in hdr and _lib.INPAINT_MAX_BLUR_RADIUS == 64
    levels = (ctypes.c_double * 2)(0.0, 100.0)
    opt = _lib.InpaintOptions(struct_size=ctypes.sizeof(_lib.InpaintOptions))
    st = lib.xfr_inpaint_iou_ex(None, None, 1, None, 1e-9, 1, 0, levels, 2, None, None, ctypes.byref(opt), None)
    assert st == _lib.XFR_INVALID_ARG and b'null engine' in lib.xfr_last_error()


@pytest.mark.skipif(shutil.which('gcc') is None, reason='needs a C compiler')
def test_options_struct_layout_matches_the_header(tmp_path):
    fields = [f for f, _ in _lib.InpaintOptions._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "xfr_amd.h"\nint main(void) {\n  printf("%zu", sizeof(xfr_inpaint_options));\n'
                   + ''.join('  printf(" %%zu", offsetof(xfr_inpaint_options, %s));\n' % f for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(_lib.InpaintOptions)] + [getattr(_lib.InpaintOptions, f).offset for f in fields]


@pytest.mark.parametrize('shape,sigma', BLUR_SHAPES)
def test_kernel_and_order_are_scipys_bit_for_bit(shape, sigma):
    w = S.gaussian_kernel1d(sigma)
    assert w.size == 2 * int(4.0 * sigma + 0.5) + 1 and np.array_equal(w, w[::-1]) and (w >= 0).all()
    m = I.bump_map(shape, seed=5)
    for q in (50, 90):
        mask = (m > np.percentile(m, q)).astype(np.float64)
        want = scipy.ndimage.gaussian_filter(mask, sigma, mode='nearest', truncate=4.0)
        assert np.array_equal(blur_in_the_kernels_order(mask, w), want), (shape, sigma, q)


@pytest.mark.parametrize('include_zero', [True, False])
@pytest.mark.parametrize('shape', [(7, 9), (37, 53), (224, 224)])
def test_percent_pixels_routing_reproduces_the_host_masks(shape, include_zero):
    """What the device is given (explicit thresholds per map, the caller's totals) decides the pixels create_threshold_masks decides."""
    rng = np.random.RandomState(shape[0])
    one = np.zeros(shape)
    one[shape[0] // 2, shape[1] // 3] = 1.0
    maps = np.stack([I.bump_map(shape, seed=3), np.maximum(rng.rand(*shape) - 0.3, 0.0), one])
    seed = 17
    np.random.seed(seed)
    noise = np.random.rand(*shape)
    for levels in (np.array([50]), np.array([0, 100]), I.STANDARD):
        thr, totals = S._pixel_thresholds(maps, levels.astype(np.float64), noise, 1e-9, include_zero)
        assert thr.shape == (3, len(levels)) and totals.shape == (3,) and (np.diff(thr, axis=1) <= 0).all()
        if levels[0] == 0:
            assert (thr[:, 0] == 1).all()
        if levels[-1] == 100:
            assert (thr[:, -1] == 0).all()
        for k, m in enumerate(maps):
            v = m + (1 if include_zero else (m != 0)) * noise * 1e-9
            got = (v / totals[k])[None] > thr[k][:, None, None]
            want = S.create_threshold_masks(m, 'percent-pixels', percentiles=levels, seed=seed, include_zero_elements=include_zero)
            assert np.array_equal(got, want), (shape, include_zero, len(levels), k)


def test_device_levels_and_blur_predicates():
    p = I.STANDARD
    assert S._device_levels('percent-density', p, None)[0] == 'percent-density'
    assert S._device_levels('percent-pixels', p, None)[0] == 'percent-pixels'
    assert S._device_levels('anything-else', p, None)[0] == 'percent-pixels'          # :57: any other name without thresholds
    assert S._device_levels('mass-threshold', None, np.array([0.5, 0.1]))[0] == 'thresholds'
    assert S._device_levels('percent-pixels', None, None) is None
    assert S._device_levels('percent-pixels', p[::-1], None) is None                    # unsorted: the host's
    assert S._device_levels('percent-density', p[::-1], None) is None
    f64 = np.float64
    assert S._device_blur(None, (224, 224), f64, p, 101) is None and S._device_blur(0, (224, 224), f64, p, 101) is None
    k, flags = S._device_blur(4, (224, 224), f64, p, 101)
    assert k.size == 2 * 36 + 1 and flags.sum() == 100 and not flags[-1]
    assert S._device_blur(4, (128, 224), f64, p, 101)[0].size == 2 * 20 + 1             # min(H, W)
    assert S._device_blur(7, (224, 224), f64, p, 101)[0].size == 2 * 63 + 1
    assert S._device_blur(8, (224, 224), f64, p, 101) is False                           # radius 72 > 64
    assert S._device_blur(4, (224, 224), np.float32, p, 101) is False                    # the reference blurs in the map's dtype
    assert S._device_blur(4, (224, 224), f64, None, 101) is False
    assert S._device_blur(0.05, (224, 224), f64, p, 101) is False                        # radius 0


def test_routing_of_the_drop_in_function(monkeypatch):
    monkeypatch.setattr(S, '_is_native', lambda snet: snet == 'native')
    monkeypatch.setattr(S, '_network_format', lambda snet, *images: all(np.shape(im) == (3, 224, 224) for im in images))
    img = np.zeros((3, 224, 224), dtype=np.float32)
    sal = I.bump_map((224, 224), seed=1)
    p = I.STANDARD

    def route(snet='native', a=img, b=img, m=sal, method='percent-density', blur=None, percentiles=p, thresholds=None):
        return S._takes_device_path(snet, a, b, m, method, blur, percentiles, thresholds)

    assert route() is not None and route()[1] is None                                   # today's conditions
    assert route(thresholds=np.array([0.5, 0.1]), method='mass-threshold', percentiles=None) is not None
    assert route(blur=4) is not None and route(blur=4)[1][0].size == 73
    assert route(method='percent-pixels')[0][0] == 'percent-pixels'
    assert route(method='percent-pixels', blur=4) is not None
    assert route(blur=4, m=sal.astype(np.float32)) is None                               # float32 map with blur
    assert route(m=sal.astype(np.float32)) is not None                                   # ... without: as today
    assert route(blur=9) is None                                                         # radius above the limit
    assert route(percentiles=p[::-1]) is None                                            # unsorted levels
    assert route(a=np.zeros((224, 224, 3), dtype=np.float32), b=np.zeros((224, 224, 3), dtype=np.float32)) is None
    assert route(blur=4, percentiles=None, thresholds=np.array([0.5, 0.1]), method='mass-threshold') is None
    assert route(method='percent-pixels', m=sal - 1.0) is None                            # negative values: thresholds may rise
    assert route(snet='other') is None
    monkeypatch.setattr(S, 'FORCE_HOST', True)
    assert route() is None and route(blur=4) is None


def test_score_maps_keeps_its_refusals():
    with pytest.raises(ValueError, match='score_maps runs on the device'):
        S.score_maps(None, None, None, None, None, np.ones((4, 4)), percentiles=I.STANDARD[::-1])
    with pytest.raises(ValueError, match='score_maps runs on the device'):
        S.score_maps(None, None, None, None, None, np.ones((4, 4)), thresholds=np.array([0.1, 0.2]), mask_threshold_method='mass-threshold')
    with pytest.raises(ValueError, match='score_maps blurs on the device'):
        S.score_maps(None, None, None, None, None, np.ones((4, 4), dtype=np.float32), percentiles=I.STANDARD, mask_blur_sigma=4)
