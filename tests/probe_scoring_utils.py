"""What the GPU tests of STRise and inpainting-game scoring share (test_gpu_strise, test_gpu_strise_wb, test_gpu_inpaint_game, test_gpu_inpaint_soft,
test_gpu_probe_sweep): the white boxes and their module-scoped fixtures, the fixture's images and draws, and the checks of scores against the
float64 reference of a golden file.  A plain module: a test module imports the fixtures it uses by name."""
import os

import numpy as np
import pytest

import inpaint_game_inputs as I
from parity_utils import make_backbone
from xfr_amd import synth
from xfr_amd.models import blackbox as BB
from xfr_amd.models import whitebox as WB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gold(name):
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_%s.npz' % name))


def whitebox(arch, batch, device, ncls=None):
    """A Whitebox of `arch` with seed-0 weights and engines of `batch` images; ncls: the fixtures' class count of the network unless given."""
    bb, _ = make_backbone(arch, seed=0, num_classes=I.NUM_CLASSES.get(arch) if ncls is None else ncls)
    bb.to(device)
    wbn = {'lightcnn29v2': WB.WhiteboxLightCNN, 'resnet50_128': WB.Whitebox_resnet50_128}.get(arch, WB.WhiteboxSTResnet)(bb)
    wbn.default_max_batch = batch
    wb = WB.Whitebox(wbn)
    wb.batch_size = batch
    return wb


@pytest.fixture(scope='module')
def mini48(gpu_device):
    return whitebox('stresnet_mini', 48, gpu_device)


@pytest.fixture(scope='module')
def mini32(gpu_device):
    return whitebox('stresnet_mini', 32, gpu_device)


@pytest.fixture(scope='module')
def lcnn(gpu_device):
    return whitebox('lightcnn29v2', 8, gpu_device)


@pytest.fixture(scope='module')
def r50(gpu_device):
    return whitebox('resnet50_128', 4, gpu_device)


@pytest.fixture(scope='module')
def images():
    """Probe (seed 1), references (2-4), gallery (5-7): the STRise fixtures' images."""
    return [synth.synth_smooth_images(1, (3, 224, 224), seed=s)[0].permute(1, 2, 0).numpy().astype(np.uint8) for s in range(1, 8)]


def noise(seed, shape):
    np.random.seed(seed)
    return np.random.rand(*shape)


# ---- STRise ----------------------------------------------------------------------------------------------------------------------------
def strise(gold, case, images, wb, **kw):
    """BB.STRise of a case of golden_strise.npz on wb, with the fixture's draws."""
    n_refs, n_gal = int(gold[case + '/n_refs']), int(gold[case + '/n_gal'])
    args = dict(probe=images[0], refs=list(images[1:1 + n_refs]), gallery=list(images[4:4 + n_gal]), black_box='resnetv4_pytorch',
                num_masks=int(gold[case + '/num_masks']), num_mask_elements=int(gold[case + '/num_mask_elements']),
                mask_fill_type=str(gold[case + '/fill']), net=wb)
    args.update(kw)
    st = BB.STRise(**args)
    st.mask_cells = gold[case + '/mask_cells'].copy()
    st.mask_shifts = gold[case + '/mask_shifts'].copy()
    st.apply_masks()
    return st


def score_error(gold, case, scores):
    """-> (the scores' error against the float64 reference, r: the float32 reference's own), both relative to the largest score."""
    s32, s64 = gold[case + '/scores32'], gold[case + '/scores64']
    top = np.abs(s64).max()
    return np.abs(np.asarray(scores) - s64).max() / top, np.abs(s32 - s64).max() / top


def reference_selection(scores, positive, percentile=0):
    """blackbox.py:424-437."""
    if positive:
        return scores >= np.percentile(scores[scores > 0], percentile)
    return -scores >= np.percentile(-scores[scores < 0], percentile)


# ---- inpainting game -------------------------------------------------------------------------------------------------------------------
def inpaint_case(gold, name):
    """A case of golden_inpaint_game.npz as the engine's arguments."""
    arch, method, levels, include_zero, _ = I.CASES[name]
    seed = int(gold[name + '/seed'])
    maps = I.maps_of(name, seed)
    return dict(arch=arch, method=method, levels=levels, include_zero=include_zero, seed=seed, maps=maps, noise=noise(seed, maps.shape[1:]))


def check_scores(gold, name, tag, cls, pg, pr, report=None):
    """Distances within 4 r of the float64 reference (r: the float32 reference's own error), no classification flip outside the excluded levels."""
    pg64, pr64, r = gold[name + '/pg64'], gold[name + '/pr64'], float(gold[name + '/r'])
    top = max(np.abs(pg64).max(), np.abs(pr64).max())
    err = max(np.abs(pg - pg64).max(), np.abs(pr - pr64).max()) / top
    keep = ~gold[name + '/excluded']
    flips = int((cls != gold[name + '/cls64'])[keep].sum())
    if report is not None:
        report['scores/%s%s' % (name, tag)] = {'rel_err_vs_ref64': float(err), 'r_ref32_vs_ref64': r, 'bar': 4 * r, 'class_flips': flips,
                                               'levels_excluded': int((~keep).sum())}
    print('%s%s distances: %.3e (r = %.3e, bar %.3e), %d classification flips, %d levels excluded' % (name, tag, err, r, 4 * r, flips, int((~keep).sum())))
    assert pg.shape == pg64.shape and pg.dtype == np.float64 and np.isfinite(pg).all() and np.isfinite(pr).all()
    assert err <= 4 * r
    assert flips == 0
    assert np.array_equal(cls, pg < pr) and not cls[:, 0].any()
