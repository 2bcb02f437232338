"""GPU tests of native inpainting-game scoring (include/xfr_amd.h: xfr_inpaint_*; xfr_amd.inpainting_score) against the real reference's CPU run
(tests/golden/golden_inpaint_game.npz, make_golden_inpaint_game.py) and against the host restatement of create_threshold_masks.

Bars (none of them taken from the code under test):
  masks           first_on equal to the fixture's and to the host restatement's, exactly.  The fixture's maps keep every cumulative value at least
                  1e-10 from every threshold, 10 x the worst float64 summation bound, so no summation order can move a pixel; the seeded maps of
                  the size sweep are checked the same way before they are compared;
  blends          bit-equal to np.where on the fp32 tensors;
  distances       max|gpu - d64| / max|d64| <= 4 r, r = max|d32 - d64| / max|d64| read from the fixture (the reference's own fp32 run is 1 r; the
                  factor 4 is the margin for another fp32 summation order: MFMA tiles, bf16x6 folds) -- the bar of tests/test_gpu_strise.py;
  classification  equal to the float64 run's on every level the fixture does not exclude (|pg64 - pr64| <= 10 r max|d64|);
  IoU counts      exact;
  drop-in         the device path against the same function on the host path (snet.embeddings): distances of unit vectors within 1e-4, the
                  forward's tolerance (tools/embeddings_sweep.py), masks and blends equal.
With XFR_INPAINT_REPORT=<file> in the environment the measured figures are written there as JSON."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import inpaint_game_inputs as I
import probe_scoring_utils as U
from probe_scoring_utils import lcnn, mini32, mini48      # noqa: F401 (fixtures)
from xfr_amd import inpainting_score as S

pytestmark = pytest.mark.gpu
GOLD = U.gold('inpaint_game')
MINI_CASES = ('mini/zero_on', 'mini/zero_off', 'mini/thresholds', 'mini/two_maps')
REPORT = {}
_whitebox, _noise, _case = U.whitebox, U.noise, functools.partial(U.inpaint_case, GOLD)
_check_scores = functools.partial(U.check_scores, GOLD, report=REPORT)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    path = os.environ.get('XFR_INPAINT_REPORT')
    if REPORT and path:
        with open(path, 'w') as f:
            json.dump(dict(sorted(REPORT.items())), f, indent=1)


def _guarded(m, levels, seed, include_zero):
    """The fixture's condition for a percent-density map: no cumulative value within 1e-10 of a positive threshold, the maximum at 1 aside."""
    s = m + (1 if include_zero else (m != 0)) * _noise(seed, m.shape) * 1e-9
    s = np.sort((s / s.sum()).ravel())
    cdf = np.cumsum(s)
    cdf = cdf / cdf.max()
    thr = 1.0 - np.asarray(levels, dtype=np.float64) / 100
    gap = np.abs(cdf[None, :-1] - thr[thr > 0][:, None])
    return gap.size == 0 or gap.min() > 1e-10


def _host_first_on(m, method, levels, seed, include_zero):
    kw = dict(percentiles=levels) if method == 'percent-density' else dict(thresholds=levels)
    masks = S.create_threshold_masks(m, method if method == 'percent-density' else 'mass-threshold', seed=seed, include_zero_elements=include_zero, **kw)
    assert (masks[1:] >= masks[:-1]).all()
    return (len(levels) - masks.sum(axis=0)).astype(np.uint8)


def _score(wb, name):
    c = _case(name)
    a, b = I.probe_pair(c['arch'])
    key = name.split('/')[0]
    eng = wb._engine(wb.batch_size)
    cls, pg, pr = eng.inpaint_score(c['maps'], c['levels'], a, b, GOLD[key + '/gal_orig'], GOLD[key + '/gal_inp'], wb.net._mark('encode'),
                                    method=c['method'], noise=c['noise'], include_zero=c['include_zero'])
    return cls.cpu().numpy().astype(bool), pg.cpu().numpy(), pr.cpu().numpy()


# ---- masks -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(I.CASES))
def test_masks_equal_the_fixture(mini48, name):
    c = _case(name)
    eng = mini48._engine(48)
    got, cdf = eng.inpaint_masks(c['maps'], c['levels'], method=c['method'], noise=c['noise'], include_zero=c['include_zero'], want_cdf=True)
    got, cdf = got.cpu().numpy(), cdf.cpu().numpy()
    wrong = int((got != GOLD[name + '/first_on']).sum())
    REPORT['masks/' + name] = {'pixels_wrong': wrong}
    assert got.dtype == np.uint8 and got.shape == c['maps'].shape
    assert wrong == 0
    if c['method'] == 'percent-density':
        assert cdf.max() == 1.0 and cdf.min() >= 0.0
    again = eng.inpaint_masks(c['maps'], c['levels'], method=c['method'], noise=c['noise'], include_zero=c['include_zero'], want_cdf=True)
    assert np.array_equal(again[1].cpu().numpy(), cdf), 'two runs differ in the float64 values'


@pytest.mark.parametrize('shape', [(7, 9), (37, 53), (128, 128), (224, 224)])
@pytest.mark.parametrize('include_zero', [True, False])
def test_masks_equal_the_host_restatement(mini48, shape, include_zero):
    eng = mini48._engine(48)
    rng = np.random.RandomState(shape[0])
    one = np.zeros(shape)
    one[shape[0] // 2, shape[1] // 3] = 1.0
    maps = np.stack([I.bump_map(shape, seed=3), np.maximum(rng.rand(*shape) - 0.25, 0.0), one])
    seed = 17
    noise = _noise(seed, shape)
    for levels in (np.array([50]), np.array([0, 100]), I.STANDARD):
        got = eng.inpaint_masks(maps, levels, noise=noise, include_zero=include_zero).cpu().numpy()
        for k in range(len(maps)):
            assert _guarded(maps[k], levels, seed, include_zero)
            want = _host_first_on(maps[k], 'percent-density', levels, seed, include_zero)
            assert np.array_equal(got[k], want), (shape, include_zero, len(levels), k, int((got[k] != want).sum()))
    total = (maps[0] + noise * 1e-9 * (1 if include_zero else (maps[0] != 0))).sum()
    thr = np.array([3.0, 0.7, 0.25, 0.0]) * maps[0].max() / total
    got = eng.inpaint_masks(maps[:1], thr, method='thresholds', noise=noise, include_zero=include_zero).cpu().numpy()
    assert np.array_equal(got[0], _host_first_on(maps[0], 'thresholds', thr, seed, include_zero))


# ---- blends ----------------------------------------------------------------------------------------------------------------------------
def test_blends_are_the_select_three_channels(mini48):
    name = 'mini/two_maps'
    c = _case(name)
    a, b = I.probe_pair(c['arch'])
    eng = mini48._engine(48)
    L = len(c['levels'])
    for first, count in ((0, 3), (95, 12), (199, 3)):      # the start, across the two maps, the end
        got = eng.inpaint_blends(c['maps'], c['levels'], a, b, noise=c['noise'], include_zero=c['include_zero'], first=first, count=count).cpu().numpy()
        for j in range(count):
            m, l = divmod(first + j, L)
            want = np.where((GOLD[name + '/first_on'][m] <= l)[None], b, a)
            assert got[j].dtype == np.float32 and np.array_equal(got[j], want), (first, j)


def test_blends_are_the_select_one_channel(lcnn):
    name = 'lcnn/zero_on'
    c = _case(name)
    a, b = I.probe_pair(c['arch'])
    got = lcnn._engine(8).inpaint_blends(c['maps'], c['levels'], a, b, noise=c['noise'], include_zero=c['include_zero']).cpu().numpy()
    want = np.where((GOLD[name + '/first_on'][0][None] <= np.arange(101)[:, None, None])[:, None], b[None], a[None])
    assert got.shape == (101, 1, 128, 128) and np.array_equal(got, want)


# ---- distances, classification, IoU ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', MINI_CASES)
def test_scores_mini(mini48, name):
    _check_scores(name, '', *_score(mini48, name))


def test_scores_lightcnn(lcnn):
    _check_scores('lcnn/zero_on', '', *_score(lcnn, 'lcnn/zero_on'))


def test_scores_resnet101(gpu_device):
    """32 levels through the full-size forward (the bf16x6 path at 32 images)."""
    wb = _whitebox('stresnet101', 32, gpu_device)
    _check_scores('r101/coarse', '', *_score(wb, 'r101/coarse'))
    wb.net._engine.close()


def test_partial_batches_are_padded_and_dropped(mini32, mini48):
    """101 hybrids: four batches of 32 (27 paddings) or three of 48 (43); both hold the bars."""
    for tag, wb in (('/batch32', mini32), ('/batch48', mini48)):
        _check_scores('mini/zero_on', tag, *_score(wb, 'mini/zero_on'))


def test_thirteen_batches_reuse_both_buffers(gpu_device):
    """101 hybrids on an engine of 8: thirteen batches, the last of five, so each of the two input buffers goes back to the side stream six times."""
    _check_scores('mini/zero_on', '/batch8', *_score(_whitebox('stresnet_mini', 8, gpu_device), 'mini/zero_on'))


@pytest.mark.parametrize('name', ['mini/zero_on', 'mini/zero_off', 'mini/thresholds', 'mini/two_maps', 'lcnn/zero_on'])
def test_iou_counts_are_exact(mini48, lcnn, name):
    c = _case(name)
    wb = lcnn if c['arch'] == 'lightcnn29v2' else mini48
    got = wb._engine(wb.batch_size).inpaint_iou(c['maps'], c['levels'], I.ground_truth(c['arch']), method=c['method'], noise=c['noise'],
                                                include_zero=c['include_zero']).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, GOLD[name + '/iou_counts'])
    kw = dict(percentiles=c['levels']) if c['method'] == 'percent-density' else dict(thresholds=c['levels'])
    iou = S.intersect_over_union_thresholded_saliency(c['maps'][0], I.ground_truth(c['arch']), c['method'], seed=c['seed'],
                                                      include_zero_elements=c['include_zero'], snet=wb, **kw)
    assert np.array_equal(iou, got[0, :, 0] / (got[0, :, 1] + 1e-9))


# ---- the drop-in function, end to end --------------------------------------------------------------------------------------------------
def test_drop_in_function_against_the_host_path(mini48):
    name = 'mini/zero_on'
    c = _case(name)
    a, b = I.probe_pair(c['arch'])
    args = (mini48, a, b, GOLD['mini/gal_orig'], GOLD['mini/gal_inp'], c['maps'][0], 'percent-density')
    kw = dict(percentiles=c['levels'], seed=c['seed'], return_transitions=True)
    dev = S.classified_as_inpainted_twin(*args, **kw)
    S.FORCE_HOST = True
    try:
        host = S.classified_as_inpainted_twin(*args, **kw)
    finally:
        S.FORCE_HOST = False
    d = max(np.abs(dev[1] - host[1]).max(), np.abs(dev[2] - host[2]).max())
    REPORT['drop_in/' + name] = {'max_abs_diff_device_vs_host_path': float(d), 'bar': 1e-4}
    print('drop-in: device against host path %.3e' % d)
    assert d <= 1e-4
    assert np.array_equal(dev[4], host[4]) and np.array_equal(dev[3], host[3]) and dev[3].dtype == np.float64
    assert np.array_equal(dev[0][~GOLD[name + '/excluded'][0]], host[0][~GOLD[name + '/excluded'][0]])
    _check_scores(name, '/drop_in', dev[0][None], dev[1][None], dev[2][None])


# ---- error paths -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(mini48):
    eng = mini48._engine(48)
    enc = mini48.net._mark('encode')
    sal = np.ones((1, 224, 224))
    img = torch.zeros((3, 224, 224))
    emb = torch.ones(512)
    ok = np.array([0.0, 50.0, 100.0])
    with pytest.raises(ValueError, match='0 levels'):
        eng.inpaint_masks(sal, np.array([]))
    with pytest.raises(ValueError, match='256 levels, a first_on byte holds 1 to 255'):
        eng.inpaint_masks(sal, np.linspace(0, 100, 256))
    with pytest.raises(ValueError, match='unsorted percentiles, 10 of level 2 after 50'):
        eng.inpaint_masks(sal, np.array([0.0, 50.0, 10.0]))
    with pytest.raises(ValueError, match=r'percentile 101 of level 1 outside \[0, 100\]'):
        eng.inpaint_iou(sal, np.array([0.0, 101.0]), np.ones((224, 224)))
    with pytest.raises(ValueError, match='unsorted thresholds'):
        eng.inpaint_masks(sal, np.array([0.1, 0.2]), method='thresholds')
    with pytest.raises(ValueError, match='method 7 is neither'):
        eng.inpaint_masks(sal, ok, method=7)
    with pytest.raises(ValueError, match='bad tensor id 100000'):
        eng.inpaint_score(sal, ok, img, img, emb, emb, 100000)
    with pytest.raises(ValueError, match='the engine input size'):
        eng.inpaint_score(np.ones((1, 128, 128)), ok, img, img, emb, emb, enc)
    with pytest.raises(ValueError, match='network format'):
        eng.inpaint_score(sal, ok, torch.zeros((1, 224, 224)), img, emb, emb, enc)
    with pytest.raises(ValueError, match=r'hybrids \[2, 2 \+ 2\) of 3'):
        eng.inpaint_blends(sal, ok, img, img, first=2, count=2)
    lib = eng.lib
    import ctypes
    levels = (ctypes.c_double * 3)(*ok)
    assert lib.xfr_inpaint_debug_masks(eng._h, None, 1, 224, 224, None, 1e-9, 1, 0, levels, 3, None, None, None) == 1
    assert b'null argument' in lib.xfr_last_error()
    torch.cuda.synchronize()
