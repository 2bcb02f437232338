"""GPU tests of saliency finishing: the kernels of finish.hip through the C ABI (xfr_finish_saliency), Engine.finish_saliency, saliency_io.finish_maps /
save_finished and the device-tensor path of inpainting_score.score_maps, on the mini network's engine.

The truth is xfr_amd.saliency_io's own host chain (finish_inputs.host_chain, create_save_smap's arithmetic unmodified).  Bars:
  totals given      (numpy's own float32 sums) sal within 1e-12 of host_chain on every shape and batch: float64 arithmetic against float64 arithmetic,
                    the bar the restatement itself meets against scipy at 8e-16;
  no totals         sal within 1e-12 of host_chain_exact_total, and within 4 r of the unmodified host_chain, r = finish_inputs.reference_r(): the
                    reference's distance from itself under the one stated substitution, computed on the CPU in the same test, never from the device;
  identity          sizes equal: the normalised map bit for bit;
  batches           map i alone and inside the batch of 33: bit-identical maps and overlays;
  overlay           against host_chain's bytes: at most 0.1 % of a map's pixels differ, none by more than one level in any channel outside a step of
                    the colour table (finish_inputs.overlay_check, with the zero step stated there); the constant map's overlay
                    equals the host's blend of the all-zero map exactly.
The constant maps (a constant, and any 1 x 1 map): create_save_smap itself stores NaN (0 / 0); the device states the all-zero map, and the truth of
those cases is finish_inputs.constant_truth (tests/test_finish_inputs.py pins both facts)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import finish_inputs as F
import inpaint_game_inputs as I
import probe_scoring_utils as U
from probe_scoring_utils import mini32      # noqa: F401 (fixture)
from xfr_amd import _lib
from xfr_amd import inpainting_score as S
from xfr_amd import saliency_io as SIO

pytestmark = pytest.mark.gpu
CASES = list(F.CASES)


@pytest.fixture(scope='module')
def eng(mini32):
    return mini32._engine(mini32.batch_size)


def _totals(name, n):
    return np.array([0.0 if F.is_constant(name) else F.numpy_total(m) for m in F.batch(name, n)[0]], dtype=np.float32)


def _finish(eng, name, n, totals, overlay=True):
    maps, probes = F.batch(name, n)
    sal, ov = eng.finish_saliency(torch.from_numpy(maps.copy()), F.CASES[name][2], probes_u8=torch.from_numpy(probes.copy()) if overlay else None,
                                  totals=_totals(name, n) if totals else None)
    assert sal.dtype == torch.float64 and sal.is_cuda and tuple(sal.shape) == (n,) + F.CASES[name][2]
    assert (ov is None) if not overlay else (ov.dtype == torch.uint8 and tuple(ov.shape) == (n,) + F.CASES[name][2] + (3,))
    return sal.cpu().numpy(), ov.cpu().numpy() if overlay else None


@pytest.mark.parametrize('n', F.BATCHES)
@pytest.mark.parametrize('name', CASES)
def test_maps_with_the_callers_totals(eng, name, n):
    got, _ = _finish(eng, name, n, totals=True, overlay=False)
    want, _ = F.truth(name, n, False)
    err = float(np.abs(got - want).max())
    print('%s n=%d: device against host_chain %.3e' % (name, n, err))
    assert np.isfinite(got).all() and err <= 1e-12


@pytest.mark.parametrize('n', F.BATCHES)
@pytest.mark.parametrize('name', CASES)
def test_maps_with_the_devices_own_total(eng, name, n):
    r = F.reference_r()
    got, _ = _finish(eng, name, n, totals=False, overlay=False)
    exact, plain = F.truth(name, n, True)[0], F.truth(name, n, False)[0]
    err, err_plain = float(np.abs(got - exact).max()), float(np.abs(got - plain).max())
    print('%s n=%d: device against host_chain_exact_total %.3e, against host_chain %.3e (r = %.3e, bar %.3e)' % (name, n, err, err_plain, r, 4 * r))
    assert np.isfinite(got).all() and err <= 1e-12
    assert err_plain <= 4 * r


@pytest.mark.parametrize('name', ['identity_112', 'identity_224'])
def test_identity_sizes_are_the_normalised_map_bit_for_bit(eng, name):
    for totals in (True, False):
        got, _ = _finish(eng, name, 3, totals=totals, overlay=False)
        want = np.stack([F.normalised(m, exact_total=not totals) for m in F.batch(name, 3)[0]])
        assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize('name', CASES)
def test_a_map_does_not_depend_on_its_batch(eng, name):
    maps, probes = F.batch(name, 33)
    sal, ov = _finish(eng, name, 33, totals=False)
    for i in (0, 16, 32):
        s1, o1 = eng.finish_saliency(torch.from_numpy(maps[i:i + 1].copy()), F.CASES[name][2], probes_u8=torch.from_numpy(probes[i:i + 1].copy()))
        assert s1.cpu().numpy().tobytes() == sal[i].tobytes() and o1.cpu().numpy().tobytes() == ov[i].tobytes()


@pytest.mark.parametrize('n', F.BATCHES)
@pytest.mark.parametrize('name', CASES)
def test_overlay_against_the_hosts_bytes(eng, name, n):
    _, got = _finish(eng, name, n, totals=True)
    sal, want = F.truth(name, n, False)
    if F.is_constant(name):
        assert np.array_equal(got, want) and np.array_equal(got, F.batch(name, n)[1])      # the image itself
        return
    worst = (0, 0, sal[0].size)
    for i in range(n):
        found = F.overlay_check(name, got[i], want[i], sal[i])
        worst = max(worst, found, key=lambda t: (t[0], t[1]))
    print('%s n=%d: at most %d of %d pixels of a map differ, %d levels apart outside table steps' % ((name, n) + (worst[0], worst[2], worst[1])))


def test_save_finished_writes_what_create_save_smap_writes(eng, tmp_path):
    name, n = 'generator', 3
    maps, probes = F.batch(name, n)
    smaps, overlays = SIO.finish_maps(eng, maps, list(probes))
    r = F.reference_r()
    for i in range(n):
        host, dev = str(tmp_path / 'host'), str(tmp_path / 'dev')
        assert SIO.create_save_smap('m', host, False, lambda i=i: maps[i], '%05d' % i, probes[i]) is True
        SIO.save_finished(dev, '%05d' % i, 'm', smaps[i], overlays[i])
        assert sorted(os.listdir(dev)) == sorted(os.listdir(host)) and len(os.listdir(dev)) == 2 * (i + 1)
        a, b = np.load(SIO.saliency_paths(host, '%05d' % i, 'm')[1]), np.load(SIO.saliency_paths(dev, '%05d' % i, 'm')[1])
        assert a.files == b.files == ['saliency_map'] and a['saliency_map'].dtype == b['saliency_map'].dtype == np.float64
        assert a['saliency_map'].shape == b['saliency_map'].shape
        assert np.abs(a['saliency_map'] - b['saliency_map']).max() <= 4 * r          # finish_maps divides by the device's own total
        assert np.abs(SIO.load_smap(dev, '%05d' % i, 'm') - F.truth(name, n, True)[0][i]).max() <= 1e-12
        import PIL.Image
        png = np.asarray(PIL.Image.open(SIO.saliency_paths(dev, '%05d' % i, 'm')[0]))
        assert np.array_equal(png, overlays[i].cpu().numpy())
        F.overlay_check(name, png, F.truth(name, n, True)[1][i], F.truth(name, n, True)[0][i])      # the host's bytes under the same total
        # the generator's resume: the files save_finished left make create_save_smap skip
        assert SIO.create_save_smap('m', dev, False, lambda: pytest.fail('recomputed'), '%05d' % i, probes[i]) is False


@pytest.mark.parametrize('method', ['percent-density', 'thresholds'])
def test_score_maps_reads_the_device_tensor(mini32, eng, method):
    """generate -> finish -> score without a host copy: the scores of the device tensor equal those of its host copy, exactly."""
    gold = U.gold('inpaint_game')
    a, b = I.probe_pair('stresnet_mini')
    maps = np.stack([F.seeded_map('field', (112, 112), s) for s in range(2)])
    sal, _ = eng.finish_saliency(torch.from_numpy(maps), (224, 224))
    kw = dict(percentiles=I.COARSE) if method == 'percent-density' else dict(thresholds=I.THRESHOLDS, mask_threshold_method='thresholds')
    args = (mini32, a, b, gold['mini/gal_orig'], gold['mini/gal_inp'])
    dev = S.score_maps(*(args + (sal,)), seed=3, **kw)
    host = S.score_maps(*(args + (sal.cpu().numpy(),)), seed=3, **kw)
    for x, y in zip(dev, host):
        assert x.shape == y.shape == (2, len(I.COARSE if method == 'percent-density' else I.THRESHOLDS)) and x.tobytes() == y.tobytes()
    with pytest.raises(ValueError, match='float64'):
        S.score_maps(*(args + (sal.float(),)), seed=3, **kw)


def test_percent_pixels_takes_the_host_copy(mini32, eng):
    gold = U.gold('inpaint_game')
    a, b = I.probe_pair('stresnet_mini')
    sal, _ = eng.finish_saliency(torch.from_numpy(F.seeded_map('field', (112, 112), 5)[None]), (224, 224))
    args = (mini32, a, b, gold['mini/gal_orig'], gold['mini/gal_inp'])
    dev = S.score_maps(*(args + (sal,)), percentiles=I.COARSE, mask_threshold_method='percent-pixels', seed=3)
    host = S.score_maps(*(args + (sal.cpu().numpy(),)), percentiles=I.COARSE, mask_threshold_method='percent-pixels', seed=3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(dev, host))


def test_a_refused_call_leaves_the_engine_usable(eng):
    maps, probes = F.batch('blocks_16x16', 3)
    want, _ = _finish(eng, 'blocks_16x16', 3, totals=False, overlay=False)
    with pytest.raises(_lib.XfrError, match='shrinking axis') as info:
        eng.finish_saliency(torch.from_numpy(maps.copy()), (48, 8))
    assert info.value.status == _lib.XFR_INVALID_ARG
    dm = torch.from_numpy(maps.copy()).to(eng.device)
    dp = torch.from_numpy(probes.copy()).to(eng.device)
    sal = torch.empty((3, 48, 40), device=eng.device, dtype=torch.float64)
    ov = torch.empty((3, 48, 40, 3), device=eng.device, dtype=torch.uint8)
    with pytest.raises(_lib.XfrError, match='without a colour table'):
        eng._finish_call(dm.data_ptr(), 3, 16, 16, 48, 40, None, dp.data_ptr(), None, sal.data_ptr(), ov.data_ptr())
    lut = (ctypes.c_double * 768)()
    with pytest.raises(_lib.XfrError, match='overlap'):
        eng._finish_call(dm.data_ptr(), 3, 16, 16, 48, 40, None, dp.data_ptr(), lut, sal.data_ptr(), dp.data_ptr())
    with pytest.raises(_lib.XfrError, match='total 1'):
        eng.finish_saliency(dm, (48, 40), totals=[1.0, -1.0, 1.0])
    got, _ = _finish(eng, 'blocks_16x16', 3, totals=False, overlay=False)
    assert got.tobytes() == want.tobytes()
