"""Host tests of saliency finishing (include/xfr_amd.h: xfr_finish_saliency; xfr_amd/csrc/finish.hip): the numpy restatement of the closed form the
kernels evaluate against scipy, the reference's distance from itself, the stability of the overlay's bytes, and the C-ABI boundary.  No device.

Bars:
  restatement   finish_inputs.spline_resize equals saliency_io._resize_cubic within 1e-12 on every shape (the bar DESIGN.md 9c uses for a restated
                scipy resample; 8e-16 is measured);
  r             the largest distance between host_chain and host_chain_exact_total, recomputed here.  A float32 pairwise sum of n values is within
                log2(n) ulp of the exact one, 14 x 6e-8 at the generator's 12544 pixels, and the normalised map is at most 1: r < 1e-6;
  overlay       reference code only: the finished map perturbed by the restatement-vs-scipy difference gives the same bytes but for at most 0.1 % of
                a map's pixels, each one level apart (3 of 301056 pixels at 224 x 224 and 8 of 215040 at 160 x 224 were found, 0 at the small shapes).
                That holds with the zero step finish_inputs.overlay_check states: where a map's true value is zero, scipy and the
                restatement differ in bytes (6 of 63 pixels of a 3 x 4 map, 122 of 1920 of the one-pixel map), every one at a value below 1e-15."""
import ctypes
import os
import re

import numpy as np
import pytest

import finish_inputs as F
from xfr_amd import _lib
from xfr_amd import saliency_io as SIO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', list(F.CASES))
def test_restatement_equals_scipy(name):
    kind, hw, HW = F.CASES[name]
    inputs = [F.resize_input(name, s) for s in range(2)]
    if not F.is_constant(name):
        inputs += [F.normalised(m) for m in F.batch(name, 3)[0]]
    worst = 0.0
    for a in inputs:
        got, want = F.spline_resize(a, HW), SIO._resize_cubic(a, HW)
        assert got.shape == want.shape == HW
        worst = max(worst, float(np.abs(got - want).max()))
    print('%s: restatement against scipy %.3e' % (name, worst))
    assert worst <= 1e-12
    if hw == HW:
        assert worst == 0.0


def test_reference_distance_from_itself():
    r = F.reference_r()
    print('r = %.3e' % r)
    assert 0.0 < r < 1e-6


def test_constant_map_is_nan_on_the_host_and_stated_on_the_device():
    """create_save_smap's 0 / 0: the reason the constant cases have a stated truth instead of host_chain's."""
    maps, probes = F.batch('constant', 1)
    with np.errstate(all='ignore'):
        assert np.isnan(F.host_chain(maps[0], probes[0])[0]).all()
    s, o = F.constant_truth(probes[0])
    assert not s.any() and np.array_equal(o, (probes[0] / 255.0 * 255).astype(np.uint8)) and np.array_equal(o, probes[0])


@pytest.mark.parametrize('name', F.VARYING)
def test_overlay_bytes_are_stable_under_the_restatement(name):
    kind, hw, HW = F.CASES[name]
    maps, probes = F.batch(name, 33 if max(HW) < 100 else 3)
    for m, probe in zip(maps, probes):
        a = F.normalised(m)
        v, w = SIO._resize_cubic(a, HW), F.spline_resize(a, HW)
        img = probe.astype(np.float64) / 255.0
        byte = lambda x: (np.clip(SIO.blend_saliency_map(img, x), 0, 1) * 255).astype(np.uint8)      # noqa: E731
        got, want = byte(w), byte(v)
        differ = int((got != want).any(axis=-1).sum())
        print('%s: %d of %d pixels differ' % (name, differ, v.size))
        F.overlay_check(name, got, want, v)
        at_zero = (got != want).any(axis=-1) & (v <= F.NOISE_FLOOR)      # the zero step: rounding residue on one side, the clip's zero on the other
        assert max(v[at_zero].max(initial=0.0), w[at_zero].max(initial=0.0)) < 1e-15


# ---- the C-ABI boundary -------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_finish_saliency():
    src = open(os.path.join(ROOT, 'include', 'xfr_amd.h')).read()
    assert re.search(r'#define XFR_AMD_ABI_VERSION 7\b', src) and _lib.ABI_VERSION == 7
    lib = _lib.load()
    assert lib.xfr_abi_version() == 7
    bound = dict((n, a) for n, _, a in _lib.SYMBOLS)
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    decl = re.search(r'xfr_status XFR_EX xfr_finish_saliency\((.*?)\);', code, flags=re.S)
    assert decl and len(decl.group(1).split(',')) == len(bound['xfr_finish_saliency']) == 13
    assert hasattr(lib, 'xfr_finish_saliency')
    assert int(re.search(r'#define XFR_FINISH_MAX_MAPS (\d+)', src).group(1)) == _lib.FINISH_MAX_MAPS
    assert int(re.search(r'#define XFR_FINISH_MAX_DIM (\d+)', src).group(1)) == _lib.FINISH_MAX_DIM
    comment = src[:src.index('xfr_status XFR_EX xfr_finish_saliency(')].rsplit('/* ----', 1)[1]
    for lines in ('show.py:196-222', ':131-137', ':46-129'):
        assert lines in comment


def test_argument_checks_that_need_no_device():
    lib = _lib.load()
    p = ctypes.c_void_p(64)      # never dereferenced: every refusal below comes before the engine or a buffer is touched
    lut = (ctypes.c_double * 768)()
    call = lambda e, h, w, H, W, probes=None, table=None, overlay=None: lib.xfr_finish_saliency(e, p, 1, h, w, H, W, None, probes, table, p, overlay, None)      # noqa: E731
    for status_of, text in ((lambda: call(None, 4, 4, 8, 8), 'null engine'),
                            (lambda: call(p, 8, 8, 4, 16), 'shrinking axis'),
                            (lambda: call(p, 8, 8, 16, 7), 'shrinking axis'),
                            (lambda: call(p, 8, 8, 16, 16, probes=ctypes.c_void_p(4096), overlay=ctypes.c_void_p(8192)), 'without a colour table'),
                            (lambda: call(p, 8, 8, 16, 16, probes=ctypes.c_void_p(4096), table=lut), 'without an overlay output'),
                            (lambda: call(p, 8, 8, 16, _lib.FINISH_MAX_DIM + 1), 'XFR_FINISH_MAX_DIM'),
                            (lambda: lib.xfr_finish_saliency(p, p, 0, 8, 8, 16, 16, None, None, None, p, None, None), 'XFR_FINISH_MAX_MAPS'),
                            (lambda: lib.xfr_finish_saliency(p, p, 1, 8, 8, 16, 16, None, None, None, None, None, None), 'null')):
        assert status_of() == _lib.XFR_INVALID_ARG
        assert text.encode() in lib.xfr_last_error(), (text, lib.xfr_last_error())
    with pytest.raises(ValueError, match='shrinking axis'):
        _lib.check(call(p, 8, 8, 4, 16))


def test_finish_maps_names_the_host_function_for_what_stays_there():
    maps = np.zeros((2, 4, 4), dtype=np.float32)
    for probes in ([np.zeros((8, 8, 3)), np.zeros((8, 8, 3))],                                           # float probes
                   [np.zeros((8, 8, 3), dtype=np.uint8), np.zeros((8, 9, 3), dtype=np.uint8)],          # two sizes
                   [np.zeros((2, 8, 3), dtype=np.uint8)] * 2,                                            # a shrinking axis
                   [np.zeros((8, 8, 3), dtype=np.uint8)]):                                               # one probe for two maps
        with pytest.raises(ValueError, match='create_save_smap'):
            SIO.finish_maps(None, maps, probes)
