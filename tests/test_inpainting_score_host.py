"""Inpainting-game scoring, the host side (no GPU): the restated create_threshold_masks equals the live reference's bit for bit (skipped where the
reference is absent) and the fixture's first_on, the IoU counts equal the fixture's, and the new C-ABI symbols are declared, bound and exported
with the ABI version unchanged.  Fixture: tests/golden/golden_inpaint_game.npz (make_golden_inpaint_game.py, the reference's own CPU run)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import inpaint_game_inputs as I
from xfr_amd import _lib
from xfr_amd import inpainting_score as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_inpaint_game.npz'))
NEW_SYMBOLS = ('xfr_inpaint_score', 'xfr_inpaint_iou', 'xfr_inpaint_debug_masks', 'xfr_inpaint_debug_blends')


def _level_args(name):
    _, method, levels, include_zero, _ = I.CASES[name]
    if method == 'percent-density':
        return 'percent-density', dict(percentiles=levels, include_zero_elements=include_zero)
    return 'mass-threshold', dict(thresholds=levels, include_zero_elements=include_zero)


def _first_on(masks):
    assert masks.dtype == bool and (masks[1:] >= masks[:-1]).all()
    return (masks.shape[0] - masks.sum(axis=0)).astype(np.uint8)


def _reference():
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import ref_import
    if not ref_import.available():
        pytest.skip('the reference is not on this machine')
    ref_import.load()
    import xfr.inpainting_game.inpainting_game as G
    return G


@pytest.mark.parametrize('method', ['percent-density', 'percent-pixels', 'mass-threshold'])
@pytest.mark.parametrize('include_zero', [True, False])
@pytest.mark.parametrize('blur', [None, 2.0])
def test_host_masks_equal_the_live_reference(method, include_zero, blur):
    G = _reference()
    m = I.bump_map((61, 47), seed=5)
    kw = dict(seed=9, include_zero_elements=include_zero, blur_sigma=blur)
    if method == 'mass-threshold':
        kw['thresholds'] = np.array([1e-3, 5e-4, 1e-4, 0.0])
        kw['percentiles'] = np.array([0, 10, 50, 100])        # read by the blur loop only (:71)
    else:
        kw['percentiles'] = np.array([0, 1, 7, 50, 93, 100])
    want = G.create_threshold_masks(m.copy(), method, **kw)
    got = S.create_threshold_masks(m.copy(), method, **kw)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    assert 0 < want.astype(bool).sum() < want.size


@pytest.mark.parametrize('name', sorted(I.CASES))
def test_host_masks_equal_the_fixture(name):
    method, kw = _level_args(name)
    seed = int(GOLD[name + '/seed'])
    for k, m in enumerate(I.maps_of(name, seed)):
        masks = S.create_threshold_masks(m, method, seed=seed, **kw)
        assert np.array_equal(_first_on(masks), GOLD[name + '/first_on'][k])


@pytest.mark.parametrize('name', sorted(I.CASES))
def test_iou_counts_equal_the_fixture(name):
    arch = I.CASES[name][0]
    method, kw = _level_args(name)
    seed = int(GOLD[name + '/seed'])
    gt = I.ground_truth(arch)
    for k, m in enumerate(I.maps_of(name, seed)):
        want = GOLD[name + '/iou_counts'][k]
        assert np.array_equal(S.iou_counts(m, gt, method, seed=seed, **kw), want)
        iou, fpos, tpos = S.intersect_over_union_thresholded_saliency(m, gt, method, seed=seed, return_fpos=True, return_tpos=True, **kw)
        assert np.array_equal(tpos, want[:, 0]) and np.array_equal(fpos, want[:, 2]) and np.array_equal(iou, want[:, 0] / (want[:, 1] + 1e-9))
        assert want[-1, 0] > 0 and want[:, 1].min() >= gt.sum()


@pytest.mark.parametrize('name', sorted(I.CASES))
def test_fixture_conditions_hold(name):
    L = len(I.CASES[name][2])
    for k in range(I.CASES[name][4]):
        pg64, pr64 = GOLD[name + '/pg64'][k], GOLD[name + '/pr64'][k]
        top = max(np.abs(pg64).max(), np.abs(pr64).max())
        r = max(np.abs(GOLD[name + '/pg32'][k] - pg64).max(), np.abs(GOLD[name + '/pr32'][k] - pr64).max()) / top
        assert r <= float(GOLD[name + '/r'])
        excluded = GOLD[name + '/excluded'][k]
        assert np.array_equal(excluded, np.abs(pg64 - pr64) <= 10 * r * top)
        assert excluded.sum() <= {101: 10, 32: 3, 5: 1}[L]
        assert not GOLD[name + '/cls64'][k][0] and not (GOLD[name + '/pg32'][k][0] < GOLD[name + '/pr32'][k][0])
        assert GOLD[name + '/cls64'][k].any(), 'the game flips to the twin at some level'


def test_ratio_mate_nonmate_saliency():
    mask = np.zeros((4, 6))
    mask[:2] = 1.0
    region = np.zeros((4, 6))
    region[:, :3] = 1.0
    assert S.ratio_mate_nonmate_saliency(mask, region) == (6 / 24.0, 6 / 24.0)
    assert S.ratio_mate_nonmate_saliency(mask, region, of_total=False) == (0.5, 0.5)


def test_new_symbols_declared_bound_exported_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, 'include', 'xfr_amd.h')).read()
    declared = set(re.findall(r'xfr_status\s+(xfr_inpaint_\w+)\s*\(', hdr))
    assert declared == set(NEW_SYMBOLS)
    bound = [n for n, _, _ in _lib.SYMBOLS]
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in bound and hasattr(lib, name)
    assert '#define XFR_AMD_ABI_VERSION 7' in hdr and _lib.ABI_VERSION == 7 and lib.xfr_abi_version() == 7
    levels = (ctypes.c_double * 2)(0.0, 100.0)
    st = lib.xfr_inpaint_iou(None, None, 1, None, 1e-9, 1, 0, levels, 2, None, None, None)
    assert st == _lib.XFR_INVALID_ARG and b'null engine' in lib.xfr_last_error()
    for fn in (S.create_threshold_masks, S.classified_as_inpainted_twin, S.intersect_over_union_thresholded_saliency, S.ratio_mate_nonmate_saliency,
               S.score_maps):
        assert callable(fn)
