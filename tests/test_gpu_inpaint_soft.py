"""GPU tests of soft-edged masks (mask_blur_sigma) and 'percent-pixels' levels in native inpainting-game scoring (include/xfr_amd.h: the _ex forms
of xfr_inpaint_*, xfr_inpaint_options, xfr_inpaint_debug_soft_masks) against the real reference's CPU run (tests/golden/golden_inpaint_soft.npz,
make_golden_inpaint_soft.py), scipy on this machine, and the host restatement of create_threshold_masks.

Bars (none of them taken from the code under test):
  soft masks      bit-equal to scipy.ndimage.gaussian_filter(mode='nearest', truncate=4.0) of the hard masks, computed here with the same weights;
                  against the fixture's stored rows <= 1e-13: two passes of at most 129 non-negative terms summing to 1 are bounded by about 3e-14,
                  and the tolerance is there only because two machines' exp may differ in the last bit of a weight;
  soft blends     bit-equal to ((1 - m) * a + m * b).astype(float32) from the scipy masks on float64 copies of the fp32 images;
  distances       max|gpu - d64| / max|d64| <= 4 r, r = max|d32 - d64| / max|d64| read from the fixture -- the bar and the reasoning of
                  tests/test_gpu_inpaint_game.py;  classification equal to the float64 run's on every level the fixture does not exclude;
  percent-pixels  first_on equal to the fixture's and the host restatement's with no guard: the device divides by the caller's total and compares
                  numpy's own values; IoU counts exact;
  drop-in         the device path against the same function on the host path: masks and blends equal, distances within 1e-4."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.ndimage
import torch

import inpaint_game_inputs as I
import inpaint_soft_inputs as J
import probe_scoring_utils as U
from probe_scoring_utils import lcnn, mini48      # noqa: F401 (fixtures)
from xfr_amd import _lib
from xfr_amd import inpainting_score as S

pytestmark = pytest.mark.gpu
GOLD = U.gold('inpaint_soft')
MINI_CASES = tuple(n for n in J.CASES if n.startswith('mini/'))
BLUR_CASES = tuple(n for n in J.CASES if J.CASES[n][5] is not None)
_whitebox, _noise, _check_scores = U.whitebox, U.noise, functools.partial(U.check_scores, GOLD)


def _request(name):
    """The engine's arguments of a fixture case, through the package's own routing: (maps, levels, keywords)."""
    arch, method, levels, include_zero, _, blur = J.CASES[name]
    seed = int(GOLD[name + '/seed'])
    maps = J.maps_of(name, seed)
    lv = S._device_levels(method, levels, None)
    b = S._device_blur(blur, maps.shape[1:], maps.dtype, levels, len(levels))
    assert lv is not None and b is not False and (b is None) == (blur is None)
    lv, kw = S._engine_request(lv, maps, _noise(seed, maps.shape[1:]), 1e-9, include_zero, b)
    return maps, lv, kw


def _scipy_masks(first_on, levels, sigma, flags=None):
    """n_levels x H x W float64: what create_threshold_masks makes of the hard masks of one map."""
    out = (first_on[None] <= np.arange(len(levels))[:, None, None]).astype(np.float64)
    for l in range(len(levels)):
        if flags is None or flags[l]:
            out[l] = scipy.ndimage.gaussian_filter(out[l], sigma, mode='nearest', truncate=4.0)
    return out


def _score(wb, name):
    maps, lv, kw = _request(name)
    a, b = I.probe_pair(J.CASES[name][0])
    key = name.split('/')[0]
    cls, pg, pr = wb._engine(wb.batch_size).inpaint_score(maps, lv, a, b, GOLD[key + '/gal_orig'], GOLD[key + '/gal_inp'], wb.net._mark('encode'), **kw)
    return cls.cpu().numpy().astype(bool), pg.cpu().numpy(), pr.cpu().numpy()


# ---- soft masks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,sigma', [((7, 9), 3.0), ((37, 53), 0.3), ((37, 53), 1.48), ((128, 128), 5.12), ((224, 224), 8.96), ((224, 224), 2.24)])
def test_soft_masks_equal_scipy(mini48, shape, sigma):
    """(7, 9) at sigma 3: radius 12 exceeds both sides, every tap clamps.  Two maps, so the second half of the list reads the second first_on."""
    eng = mini48._engine(48)
    rng = np.random.RandomState(shape[0])
    maps = np.stack([I.bump_map(shape, seed=3), np.maximum(rng.rand(*shape) - 0.25, 0.0)])
    noise = _noise(17, shape)
    w = S.gaussian_kernel1d(sigma)
    for levels in (np.array([50]), np.array([0, 100]), I.STANDARD):
        first_on = eng.inpaint_masks(maps, levels, noise=noise).cpu().numpy()
        for flags in ((levels != 100), None) if len(levels) == 2 else ((levels != 100),):
            got = eng.inpaint_soft_masks(maps, levels, noise=noise, blur_kernel=w, blur_levels=flags).cpu().numpy()
            assert got.dtype == np.float64 and got.shape == (2 * len(levels),) + shape
            for k in range(2):
                want = _scipy_masks(first_on[k], levels, sigma, flags)
                mine = got[k * len(levels):(k + 1) * len(levels)]
                assert np.array_equal(mine, want), (shape, sigma, len(levels), k, float(np.abs(mine - want).max()))
                if flags is not None and levels[-1] == 100:
                    assert set(np.unique(mine[-1])) <= {0.0, 1.0}                        # level 100 stays 0 / 1 exactly
    hard = eng.inpaint_soft_masks(maps, I.STANDARD, noise=noise, first=95, count=12).cpu().numpy()      # no options: the hard masks
    first_on = eng.inpaint_masks(maps, I.STANDARD, noise=noise).cpu().numpy()
    for j in range(12):
        m, l = divmod(95 + j, 101)
        assert np.array_equal(hard[j], (first_on[m] <= l).astype(np.float64))


@pytest.mark.parametrize('name', BLUR_CASES)
def test_soft_masks_against_the_fixture_rows(mini48, name):
    maps, lv, kw = _request(name)
    L = len(J.CASES[name][2])
    rows = GOLD[name + '/soft_rows']
    worst = 0.0
    for k in range(len(maps)):
        for j, l in enumerate(GOLD[name + '/soft_levels']):
            got = mini48._engine(48).inpaint_soft_masks(maps, lv, first=k * L + int(l), count=1, **kw).cpu().numpy()[0]
            worst = max(worst, float(np.abs(got[rows] - GOLD[name + '/soft'][k, j]).max()))
    print('%s soft masks against the reference rows: %.3e' % (name, worst))
    assert worst <= 1e-13


# ---- soft blends -----------------------------------------------------------------------------------------------------------------------
def test_soft_blends_three_channels(mini48):
    eng = mini48._engine(48)
    a, b = I.probe_pair('stresnet_mini')
    maps = J.maps_of('mini/two_maps_pixels', 200)
    noise = _noise(200, maps.shape[1:])
    levels, sigma = I.STANDARD, 8.96
    flags = levels != 100
    first_on = eng.inpaint_masks(maps, levels, noise=noise).cpu().numpy()
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for first, count in ((0, 3), (95, 12), (199, 3)):      # the start, across the two maps, the end (level 100 of the second map: hard)
        got = eng.inpaint_blends(maps, levels, a, b, noise=noise, first=first, count=count, blur_kernel=S.gaussian_kernel1d(sigma),
                                 blur_levels=flags).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (count, 3, 224, 224)
        for j in range(count):
            k, l = divmod(first + j, 101)
            m = (first_on[k] <= l).astype(np.float64)
            if flags[l]:
                m = scipy.ndimage.gaussian_filter(m, sigma, mode='nearest', truncate=4.0)
            want = ((1.0 - m[None]) * a64 + m[None] * b64).astype(np.float32)
            assert np.array_equal(got[j], want), (first, j, float(np.abs(got[j] - want).max()))


def test_soft_blends_one_channel(lcnn):
    eng = lcnn._engine(8)
    a, b = I.probe_pair('lightcnn29v2')
    maps = J.maps_of('lcnn/blur4', 200)
    noise = _noise(200, maps.shape[1:])
    levels, sigma = I.STANDARD, 5.12
    flags = levels != 100
    first_on = eng.inpaint_masks(maps, levels, noise=noise).cpu().numpy()[0]
    got = eng.inpaint_blends(maps, levels, a, b, noise=noise, blur_kernel=S.gaussian_kernel1d(sigma), blur_levels=flags).cpu().numpy()
    m = _scipy_masks(first_on, levels, sigma, flags)[:, None]
    want = ((1.0 - m) * a.astype(np.float64)[None] + m * b.astype(np.float64)[None]).astype(np.float32)
    assert got.shape == (101, 1, 128, 128) and np.array_equal(got, want)


def test_blur_flags_all_zero_are_the_existing_blends(mini48):
    eng = mini48._engine(48)
    a, b = I.probe_pair('stresnet_mini')
    maps = J.maps_of('mini/two_maps_pixels', 200)
    noise = _noise(200, maps.shape[1:])
    for first, count in ((0, 3), (95, 12), (199, 3)):
        plain = eng.inpaint_blends(maps, I.STANDARD, a, b, noise=noise, first=first, count=count)
        soft = eng.inpaint_blends(maps, I.STANDARD, a, b, noise=noise, first=first, count=count, blur_kernel=S.gaussian_kernel1d(8.96),
                                  blur_levels=np.zeros(101))
        assert torch.equal(plain, soft)


# ---- scores ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', MINI_CASES)
def test_scores_mini(mini48, name):
    _check_scores(name, '', *_score(mini48, name))


def test_scores_lightcnn(lcnn):
    _check_scores('lcnn/blur4', '', *_score(lcnn, 'lcnn/blur4'))


def test_scores_resnet101(gpu_device):
    wb = _whitebox('stresnet101', 32, gpu_device)
    _check_scores('r101/coarse_blur4', '', *_score(wb, 'r101/coarse_blur4'))
    wb.net._engine.close()


def test_padding_and_buffer_reuse(mini48, gpu_device):
    """101 blurred hybrids in batches of 32 (27 paddings), 48 (43) and 8 (thirteen batches: each input buffer goes back to the side stream six
    times).  All hold the bars, and agree with each other to 4 r."""
    name = 'mini/blur4'
    runs = {48: _score(mini48, name)}
    for batch in (32, 8):
        runs[batch] = _score(_whitebox('stresnet_mini', batch, gpu_device), name)
    for batch, got in runs.items():
        _check_scores(name, '/batch%d' % batch, *got)
    r = float(GOLD[name + '/r'])
    top = max(np.abs(GOLD[name + '/pg64']).max(), np.abs(GOLD[name + '/pr64']).max())
    for x, y in ((48, 32), (48, 8), (32, 8)):
        d = max(np.abs(runs[x][1] - runs[y][1]).max(), np.abs(runs[x][2] - runs[y][2]).max()) / top
        print('batch %d against %d: %.3e (bar %.3e)' % (x, y, d, 4 * r))
        assert d <= 4 * r


# ---- percent-pixels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['mini/pixels', 'mini/pixels_blur4', 'mini/two_maps_pixels'])
def test_percent_pixels_masks_equal_the_fixture(mini48, name):
    maps, lv, kw = _request(name)
    kw = {k: v for k, v in kw.items() if not k.startswith('blur')}
    got = mini48._engine(48).inpaint_masks(maps, lv, **kw).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, GOLD[name + '/first_on'])


@pytest.mark.parametrize('shape', [(7, 9), (37, 53), (128, 128), (224, 224)])
@pytest.mark.parametrize('include_zero', [True, False])
def test_percent_pixels_masks_equal_the_host_restatement(mini48, shape, include_zero):
    """A map with 30 % exact zeros, a random one, a one-hot one; no guard band: thresholds may equal elements of s."""
    eng = mini48._engine(48)
    rng = np.random.RandomState(shape[0])
    one = np.zeros(shape)
    one[shape[0] // 2, shape[1] // 3] = 1.0
    maps = np.stack([I.bump_map(shape, seed=3), np.maximum(rng.rand(*shape) - 0.25, 0.0), one])
    assert abs((maps[0] == 0).mean() - 0.3) < 0.02
    seed = 17
    noise = _noise(seed, shape)
    for levels in (np.array([50]), np.array([0, 100]), I.STANDARD):
        thr, totals = S._pixel_thresholds(maps, levels.astype(np.float64), noise, 1e-9, include_zero)
        got = eng.inpaint_masks(maps, thr, method='thresholds', noise=noise, include_zero=include_zero, totals=totals, levels_per_map=True).cpu().numpy()
        for k in range(len(maps)):
            masks = S.create_threshold_masks(maps[k], 'percent-pixels', percentiles=levels, seed=seed, include_zero_elements=include_zero)
            assert (masks[1:] >= masks[:-1]).all()
            want = (len(levels) - masks.sum(axis=0)).astype(np.uint8)
            assert np.array_equal(got[k], want), (shape, include_zero, len(levels), k, int((got[k] != want).sum()))


def test_percent_pixels_iou_counts_are_exact(mini48):
    name = 'mini/pixels'
    maps, lv, kw = _request(name)
    gt = I.ground_truth('stresnet_mini')
    got = mini48._engine(48).inpaint_iou(maps, lv, gt, **kw).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, GOLD[name + '/iou_counts'])
    seed = int(GOLD[name + '/seed'])
    assert np.array_equal(S.iou_counts(maps[0], gt, 'percent-pixels', percentiles=I.STANDARD, seed=seed, snet=mini48), got[0])
    masks = S.create_threshold_masks(maps[0], 'percent-pixels', percentiles=I.STANDARD, seed=seed)
    assert np.array_equal(got[0, :, 0], (gt[None] & masks).sum(axis=(1, 2))) and np.array_equal(got[0, :, 1], (gt[None] | masks).sum(axis=(1, 2)))


# ---- the drop-in function, end to end --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['mini/blur4', 'mini/pixels'])
def test_drop_in_function_against_the_host_path(mini48, name):
    _, method, levels, include_zero, _, blur = J.CASES[name]
    seed = int(GOLD[name + '/seed'])
    a, b = I.probe_pair('stresnet_mini')
    m = J.maps_of(name, seed)[0]
    args = (mini48, a, b, GOLD['mini/gal_orig'], GOLD['mini/gal_inp'], m, method)
    kw = dict(percentiles=levels, seed=seed, mask_blur_sigma=blur, include_zero_elements=include_zero, return_transitions=True)
    assert S._takes_device_path(mini48, a, b, m, method, blur, levels, None) is not None
    dev = S.classified_as_inpainted_twin(*args, **kw)
    S.FORCE_HOST = True
    try:
        host = S.classified_as_inpainted_twin(*args, **kw)
    finally:
        S.FORCE_HOST = False
    d = max(np.abs(dev[1] - host[1]).max(), np.abs(dev[2] - host[2]).max())
    print('%s drop-in: device against host path %.3e' % (name, d))
    assert d <= 1e-4
    assert dev[4].dtype == host[4].dtype and np.array_equal(dev[4], host[4])
    assert dev[3].dtype == np.float64 and np.array_equal(dev[3], host[3])
    keep = ~GOLD[name + '/excluded'][0]
    assert np.array_equal(dev[0][keep], host[0][keep])
    _check_scores(name, '/drop_in', dev[0][None], dev[1][None], dev[2][None])


def test_float32_map_with_blur_takes_the_host_path(mini48):
    name = 'mini/blur4'
    seed = int(GOLD[name + '/seed'])
    a, b = I.probe_pair('stresnet_mini')
    m = J.maps_of(name, seed)[0].astype(np.float32)
    levels = np.array([0, 50, 100])
    assert S._takes_device_path(mini48, a, b, m, 'percent-density', 4, levels, None) is None
    cls, pg, pr, blends, masks = S.classified_as_inpainted_twin(mini48, a, b, GOLD['mini/gal_orig'], GOLD['mini/gal_inp'], m, 'percent-density',
                                                                mask_blur_sigma=4, percentiles=levels, seed=seed, return_transitions=True)
    assert masks.dtype == np.float32 and masks.shape == (3, 224, 224) and ((masks[1] > 0) & (masks[1] < 1)).any()
    assert pg.shape == (3,) and np.isfinite(pg).all() and np.isfinite(pr).all() and not cls[0]


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_bad_options_are_refused_before_any_launch(mini48):
    eng = mini48._engine(48)
    sal = np.ones((1, 224, 224))
    img = torch.zeros((3, 224, 224))
    ok = np.array([0.0, 50.0, 100.0])
    good = S.gaussian_kernel1d(2.0)
    with pytest.raises(ValueError, match=r'blur_radius 65 outside \[0, 64\]'):
        eng.inpaint_blends(sal, ok, img, img, blur_kernel=np.ones(131) / 131)
    skew = good.copy()
    skew[0] *= 2
    with pytest.raises(ValueError, match='asymmetric blur kernel'):
        eng.inpaint_blends(sal, ok, img, img, blur_kernel=skew)
    nan = good.copy()
    nan[3] = np.nan
    with pytest.raises(ValueError, match='blur weight -?nan at tap 3'):
        eng.inpaint_soft_masks(sal, ok, blur_kernel=nan)
    with pytest.raises(ValueError, match='blur weight -0.5 at tap 0'):
        eng.inpaint_soft_masks(sal, ok, blur_kernel=np.array([-0.5, 2.0, -0.5]))
    with pytest.raises(ValueError, match='total 0 of map 0'):
        eng.inpaint_masks(sal, ok, totals=[0.0])
    with pytest.raises(ValueError, match='total inf of map 0'):
        eng.inpaint_masks(sal, ok, totals=[np.inf])
    with pytest.raises(ValueError, match='blur_radius 8, this call is defined on hard masks'):
        eng.inpaint_iou(sal, ok, np.ones((224, 224)), blur_kernel=good)
    with pytest.raises(ValueError, match='unsorted percentiles, 10 of level 2 after 50'):
        eng.inpaint_masks(np.ones((2, 224, 224)), np.array([[0.0, 50.0, 100.0], [0.0, 50.0, 10.0]]), levels_per_map=True)
    with pytest.raises(ValueError, match='method 7 is neither'):
        eng.inpaint_masks(sal, ok, method=7, totals=[1.0])
    lib = eng.lib
    levels = (ctypes.c_double * 3)(*ok)
    out = torch.empty((1, 224, 224), device=eng.device, dtype=torch.uint8)
    sal_dev = torch.ones((1, 224, 224), device=eng.device, dtype=torch.float64)
    opt = _lib.InpaintOptions(struct_size=ctypes.sizeof(_lib.InpaintOptions) - 8)
    call = lambda o: lib.xfr_inpaint_debug_masks_ex(eng._h, sal_dev.data_ptr(), 1, 224, 224, None, 1e-9, 1, 0, levels, 3, out.data_ptr(), None, ctypes.byref(o),
                                                    None)
    assert call(opt) == _lib.XFR_INVALID_ARG
    assert b'struct_size %d' % (ctypes.sizeof(_lib.InpaintOptions) - 8) in lib.xfr_last_error()
    opt = _lib.InpaintOptions(struct_size=ctypes.sizeof(_lib.InpaintOptions), blur_radius=3)
    assert call(opt) == _lib.XFR_INVALID_ARG and b'blur_radius 3' in lib.xfr_last_error()
    opt = _lib.InpaintOptions(struct_size=ctypes.sizeof(_lib.InpaintOptions), blur_radius=3)
    blends = torch.empty((1, 3, 224, 224), device=eng.device, dtype=torch.float32)
    img_dev = img.to(eng.device)
    st = lib.xfr_inpaint_debug_blends_ex(eng._h, sal_dev.data_ptr(), 1, None, 1e-9, 1, 0, levels, 3, img_dev.data_ptr(), img_dev.data_ptr(), 0, 1,
                                         blends.data_ptr(), ctypes.byref(opt), None)
    assert st == _lib.XFR_INVALID_ARG and b'blur_radius 3 without blur_kernel_host' in lib.xfr_last_error()
    torch.cuda.synchronize()
    # flags with a radius of 0 are accepted and ignored
    plain = eng.inpaint_blends(sal, ok, img, img)
    assert torch.equal(eng.inpaint_blends(sal, ok, img, img, blur_levels=np.array([1, 0, 1])), plain)
    torch.cuda.synchronize()


# ---- existing behaviour ----------------------------------------------------------------------------------------------------------------
def test_default_options_are_the_plain_call_bit_for_bit(mini48, monkeypatch):
    eng = mini48._engine(48)
    arch, method, levels, include_zero, _ = I.CASES['mini/zero_on']
    maps = I.maps_of('mini/zero_on', 200)
    a, b = I.probe_pair(arch)
    args = (maps, levels, a, b, GOLD['mini/gal_orig'], GOLD['mini/gal_inp'], mini48.net._mark('encode'))
    kw = dict(method=method, noise=_noise(200, maps.shape[1:]), include_zero=include_zero)
    plain = eng.inpaint_score(*args, **kw)
    opt = _lib.InpaintOptions(struct_size=ctypes.sizeof(_lib.InpaintOptions))
    calls = []
    monkeypatch.setattr(eng, '_inpaint_options', lambda n_maps, lv, *a_, **k_: (calls.append(1), (ctypes.byref(opt), len(lv), (opt,)))[1])
    ex = eng.inpaint_score(*args, **kw)
    assert calls == [1]
    for x, y in zip(plain, ex):
        assert torch.equal(x, y)
