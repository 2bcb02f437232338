"""STRise blackbox saliency, the host side (no GPU): the mirror draws what the reference drew, the closed-form mask law is scipy's zoom, the
selection is the reference's, the constructor fails with the reference's strings, and the new C-ABI symbols are declared, bound and exported
with the ABI version unchanged.  Fixture: tests/golden/golden_strise.npz (make_golden_strise.py, the reference's own CPU run)."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.ndimage

from xfr_amd import _lib
from xfr_amd.models import blackbox as BB
from xfr_amd.saliency_io import resize_linear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_strise.npz'))
MINI_CASES = ('mini/e1', 'mini/e40', 'mini/bcast', 'mini/neg', 'mini/gray')
ALL_CASES = MINI_CASES + ('r101/e1',)
NEW_SYMBOLS = ('xfr_strise_score', 'xfr_strise_combine', 'xfr_strise_debug_masks', 'xfr_strise_debug_masked_probes')


def _strise(case, **kw):
    probe = np.zeros((224, 224, 3), dtype=np.uint8)
    probe[0, 0, 0] = 255
    args = dict(probe=probe, refs=[probe], gallery=[probe], black_box='resnetv4_pytorch', num_masks=int(GOLD[case + '/num_masks']),
                num_mask_elements=int(GOLD[case + '/num_mask_elements']), mask_fill_type=str(GOLD[case + '/fill']))
    args.update(kw)
    return BB.STRise(**args)


@pytest.mark.parametrize('case', ALL_CASES)
def test_mirror_draws_what_the_reference_drew(case):
    """All choice calls first, then the (x, y) pairs: after the fixture's np.random.seed the cells and shifts are the reference's, exactly."""
    st = _strise(case)
    st.prior = resize_linear(GOLD[case.split('/')[0] + '/P_prior'], (224, 224))
    np.random.seed(int(GOLD[case + '/seed']))
    st.generate_sparse_masks()
    assert st.mask_cells.dtype == np.int32 and st.mask_shifts.dtype == np.int32
    assert np.array_equal(st.mask_cells, GOLD[case + '/mask_cells'])
    assert np.array_equal(st.mask_shifts, GOLD[case + '/mask_shifts'])


@pytest.mark.parametrize('g,size', [(19, 224), (11, 128)])
def test_closed_form_mask_law_is_scipy_zoom(g, size):
    """19 x 19 -> 236 and 11 x 11 -> 140: corners, edges (the mirror fold) and interior cells, every shift on the diagonal and two off it."""
    scale = 12
    rng = np.random.RandomState(3)
    for n_elem in (1, 40):
        grid = np.ones((g, g))
        grid.ravel()[rng.choice(g * g, n_elem, replace=False)] = 0.0
        grid[0, 0] = grid[0, g - 1] = grid[g - 1, 0] = grid[g - 1, g - 1] = 0.0
        grid[0, g // 2] = grid[g - 1, g // 3] = grid[g // 2, 0] = grid[g // 3, g - 1] = 0.0
        want = scipy.ndimage.zoom(grid, (size + scale) / float(g), order=1, mode='mirror', grid_mode=True)
        assert want.shape == (size + scale, size + scale)
        for x, y in [(s, s) for s in range(scale)] + [(0, 11), (7, 2)]:
            got = BB.mask_law(grid, (size, size), scale, (x, y))
            d = np.abs(got - want[x:x + size, y:y + size]).max()
            assert d <= 1e-12, (n_elem, x, y, d)


def _reference_selection(scores, positive_scores, percentile):
    """What blackbox.py:424-437 selects, worked out by hand: the masks whose score, on the branch's side of zero, reaches the linearly
    interpolated percentile of that side's magnitudes."""
    side = np.sort(scores[scores > 0]) if positive_scores else np.sort(-scores[scores < 0])
    at = (len(side) - 1) * percentile / 100.0
    lo = int(np.floor(at))
    hi = min(lo + 1, len(side) - 1)
    threshold = side[lo] + (side[hi] - side[lo]) * (at - lo)
    return (scores if positive_scores else -scores) >= threshold


@pytest.mark.parametrize('case', ALL_CASES)
@pytest.mark.parametrize('percentile', [0, 50])
def test_selection_is_the_references_on_both_branches(case, percentile):
    st = _strise(case)
    s64 = GOLD[case + '/scores64']
    assert (s64 > 0).any() and (s64 < 0).any(), 'the fixture has scores of both signs in every case'
    for positive in (True, False):
        st.mask_scores = s64.copy()
        sel, sign = st.select_masks(positive_scores=positive, percentile=percentile)
        assert sign == (1 if positive else -1)
        assert np.array_equal(sel, _reference_selection(s64, positive, percentile))
        assert 0 < sel.sum() < len(s64)
        if percentile == 0:      # the fixture's condition: the sign-based selection does not hinge on rounding
            st.mask_scores = GOLD[case + '/scores32'].copy()
            assert np.array_equal(st.select_masks(positive_scores=positive, percentile=0)[0], sel)


@pytest.mark.parametrize('case', ALL_CASES)
def test_fixture_condition_holds(case):
    """Every |ref64 score| is at least 10 r max|ref64|, and ref32 and ref64 agree in sign."""
    s32, s64 = GOLD[case + '/scores32'], GOLD[case + '/scores64']
    top = np.abs(s64).max()
    r = np.abs(s32 - s64).max() / top
    assert np.abs(s64).min() >= 10 * r * top
    assert np.array_equal(np.sign(s32), np.sign(s64))


def test_constructor_errors_are_the_references():
    probe = np.full((224, 224, 3), 7, dtype=np.uint8)
    ok = dict(probe=probe, refs=[probe], gallery=[probe], black_box='resnetv4_pytorch')

    def msg(**kw):
        args = dict(ok)
        args.update(kw)
        with pytest.raises((ValueError, TypeError)) as ei:
            BB.STRise(**args)
        return str(ei.value)
    assert msg(probe=None) == 'Probe and reference must be specified'
    assert msg(refs=None) == 'Probe and reference must be specified'
    assert msg(probe=3) == 'Probe must be a filepath to an image or a NumPy array'
    assert msg(refs=3) == 'Refs must be a list of filepaths, NumPy arrays, or a Pandas dataframe'
    assert msg(prior_type='x') == 'Specified prior "x" is not supported'
    assert msg(prior_type=None) == 'Prior must be specified'
    assert msg(gallery=3) == 'Gallery must be a list of filepaths, NumPy arrays, or a Pandas dataframe'
    assert msg(potential_gallery=3) == 'Potential gallery must be a list of filepaths, NumPy arrays, or a Pandas dataframe'
    assert msg(black_box=None) == 'Black box name or function must be specified'
    assert msg(black_box='x') == 'Specified black box "x" is not supported'
    assert msg(mask_type='x') == 'Specified mask type "x" is not supported'
    assert msg(mask_type=None) == 'Mask type must be specified'
    assert msg(mask_fill_type='x') == 'Specified mask fill type "x" is not supported'
    assert msg(mask_fill_type=None) == 'Mask fill type must be specified'
    assert msg(triplet_score_type='x') == 'Specified triplet score type "x" is not supported.'
    assert msg(triplet_score_type=None) == 'Triplet score type must be specified'
    st = BB.STRise(**ok)
    assert (st.num_masks, st.num_mask_elements, st.mask_scale, st.mask_fill_type, st.prior_type, st.gallery_size) == (6500, 1, 12, 'blur', 'mean_ebp', 1)
    assert BB.STRise(probe=probe, refs=[probe], black_box_fn=lambda p, g: None).gallery_size == 50
    with pytest.raises(ValueError, match='Specified black box "y" is not supported'):
        st.set_black_box('y')


def test_fills_are_the_references_lines():
    probe = (np.arange(224 * 224 * 3) % 251).astype(np.uint8).reshape(224, 224, 3)
    st = BB.STRise(probe=probe, refs=[probe], black_box='resnetv4_pytorch')
    st.mask_fill_gray()
    assert st.fill_image.dtype == np.float64 and (st.fill_image == 0.5).all()
    st.mask_fill_blur()
    want = np.stack([scipy.ndimage.gaussian_filter(probe[..., c].astype(np.float64), 8.96, mode='nearest', truncate=4.0) for c in range(3)], axis=2)
    assert np.abs(st.fill_image - want).max() <= 1e-9


def test_new_symbols_declared_bound_exported_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, 'include', 'xfr_amd.h')).read()
    declared = set(re.findall(r'xfr_status\s+(xfr_strise_\w+)\s*\(', hdr))
    assert declared == set(NEW_SYMBOLS)
    bound = [n for n, _, _ in _lib.SYMBOLS]
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in bound and hasattr(lib, name)
    assert '#define XFR_AMD_ABI_VERSION 7' in hdr and _lib.ABI_VERSION == 7 and lib.xfr_abi_version() == 7
    geom = _lib.StriseGeometry(19, 19, 12, 1)
    st = lib.xfr_strise_combine(None, None, 1, None, None, 1, ctypes.byref(geom), 1, None, None)
    assert st == _lib.XFR_INVALID_ARG and b'null engine' in lib.xfr_last_error()
