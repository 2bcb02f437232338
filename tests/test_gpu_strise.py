"""GPU tests of native STRise blackbox saliency (include/xfr_amd.h: xfr_strise_*; xfr_amd.models.blackbox.STRise) against the real reference's
CPU run (tests/golden/golden_strise.npz, make_golden_strise.py) and against scipy's zoom.

Bars (none of them taken from the code under test):
  masks          max|d| <= 1e-12 against scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True): two float64 evaluations of a piecewise-linear
                 function with values in [0, 1];
  network input  max|d| <= 2**-15 against the reference's expression in numpy: one fp32 ulp for magnitudes in [128, 256), the largest a pixel
                 minus its mean reaches -- a double-rounding difference and nothing more.  Per-tensor float64 sums agree with the fixture's to
                 1e-9 relative where both sides are float64: the reference's expression on the DEVICE's float64 masks.  The fp32 tensor's own
                 sum cannot hold 1e-9: an unmasked pixel is an integer minus the channel mean, its fp32 rounding error depends on the binade
                 alone and does not average out (measured 2.0e-8 relative, 0.2 absolute, on a tensor that equals the reference's own
                 .float() tensor bit for bit); it is held to the format's bound, half an ulp of [128, 256) per element, 3 x 224 x 224 x 2**-17;
  scores         max|gpu - ref64| / max|ref64| <= 4 r, r = max|ref32 - ref64| / max|ref64| read from the fixture (the reference's own fp32 run
                 is 1 r; the factor 4 is the margin for another fp32 summation order: MFMA tiles, bf16x6 folds);
  map            <= 1e-6 against the fixture's float64-run map given the FIXTURE's scores (the merge kernel alone; float32-stored goldens of a
                 [0, 1] map), <= 4 x the fixture's ref32-to-ref64 map distance given the engine's own scores.
With XFR_STRISE_REPORT=<file> in the environment the measured figures are written there as JSON (profiles/r8/strise_parity.json is such a file)."""
import functools
import json
import os

import numpy as np
import pytest
import scipy.ndimage
import torch

import probe_scoring_utils as U
from probe_scoring_utils import images, lcnn, mini32, mini48      # noqa: F401 (fixtures)
from xfr_amd.models import blackbox as BB
from xfr_amd.models.resnet import MEAN_RGB

pytestmark = pytest.mark.gpu
GOLD = U.gold('strise')
MINI_CASES = ('mini/e1', 'mini/e40', 'mini/bcast', 'mini/neg', 'mini/gray')
SCALE = 12
REPORT = {}
_whitebox, _reference_selection = U.whitebox, U.reference_selection
_strise, _score_error = functools.partial(U.strise, GOLD), functools.partial(U.score_error, GOLD)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    path = os.environ.get('XFR_STRISE_REPORT')
    if REPORT and path:
        with open(path, 'w') as f:
            json.dump(dict(sorted(REPORT.items())), f, indent=1)


def _zoom_masks(cells, shifts, g, size):
    out = np.empty((len(cells), size, size))
    for k in range(len(cells)):
        grid = np.ones(g * g)
        grid[cells[k]] = 0.0
        full = scipy.ndimage.zoom(grid.reshape(g, g), (size + SCALE) / float(g), order=1, mode='mirror', grid_mode=True)
        out[k] = full[shifts[k, 0]:shifts[k, 0] + size, shifts[k, 1]:shifts[k, 1] + size]
    return out


def _edge_cells(g, n_masks, n_elem, seed):
    """Corners and edges first (the mirror fold), then random cells; shifts (0, 0), (11, 11), then random."""
    rng = np.random.RandomState(seed)
    special = [0, g - 1, g * (g - 1), g * g - 1, g // 2, g * (g - 1) + g // 3, g * (g // 2), g * (g // 3) + g - 1]
    cells = np.empty((n_masks, n_elem), dtype=np.int32)
    for k in range(n_masks):
        first = special[k % len(special)]
        rest = rng.choice([c for c in range(g * g) if c != first], n_elem - 1, replace=False)
        cells[k] = np.concatenate([[first], rest])
    shifts = rng.randint(0, SCALE, size=(n_masks, 2)).astype(np.int32)
    shifts[0] = (0, 0)
    shifts[1] = (SCALE - 1, SCALE - 1)
    shifts[2] = (0, SCALE - 1)
    return cells, shifts


def _reference_map(scores, sel, masks, sign):
    """blackbox.py:416-441 in numpy."""
    comb = (scores[sel][:, None, None] * masks[sel]).mean(axis=0)
    m = 1.0 - comb if sign > 0 else comb - 1.0
    m = m - m.min()
    return m / m.max()


# ---- masks -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_elem', [1, 40])
def test_masks_224_equal_scipy_zoom(mini48, n_elem):
    eng = mini48._engine(48)
    cells, shifts = _edge_cells(19, 37, n_elem, seed=n_elem)
    got = eng.strise_masks(cells, shifts, (19, 19), SCALE).cpu().numpy()
    d = np.abs(got - _zoom_masks(cells, shifts, 19, 224)).max()
    REPORT['masks/224/e%d' % n_elem] = {'max_abs_diff': float(d), 'bar': 1e-12}
    print('masks 224, %d elements: max|d| = %.3e' % (n_elem, d))
    assert got.shape == (37, 224, 224) and d <= 1e-12
    part = eng.strise_masks(cells, shifts, (19, 19), SCALE, first=5, count=3).cpu().numpy()
    assert np.array_equal(part, got[5:8])


@pytest.mark.parametrize('n_elem', [1, 40])
def test_masks_128_equal_scipy_zoom(lcnn, n_elem):
    eng = lcnn._engine(8)
    cells, shifts = _edge_cells(11, 37, n_elem, seed=10 + n_elem)
    got = eng.strise_masks(cells, shifts, (11, 11), SCALE).cpu().numpy()
    d = np.abs(got - _zoom_masks(cells, shifts, 11, 128)).max()
    REPORT['masks/128/e%d' % n_elem] = {'max_abs_diff': float(d), 'bar': 1e-12}
    print('masks 128, %d elements: max|d| = %.3e' % (n_elem, d))
    assert got.shape == (37, 128, 128) and d <= 1e-12


# ---- network input ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['mini/e1', 'mini/e40', 'mini/gray'])
def test_network_input_is_the_references_expression(mini48, images, case):
    st = _strise(case, images, mini48)
    eng = mini48._engine(48)
    cells, shifts = st.mask_cells, st.mask_shifts
    masks = _zoom_masks(cells, shifts, 19, 224)
    got = eng.strise_masked_probes(torch.from_numpy(st.probe), torch.from_numpy(st.fill_image), cells, shifts, (19, 19), SCALE).cpu().numpy()
    dev_masks = eng.strise_masks(cells, shifts, (19, 19), SCALE).cpu().numpy()
    worst, worst_sum, worst_sum32 = 0.0, 0.0, 0.0
    for k in range(len(cells)):
        masked = masks[k][..., None] * st.probe + (1.0 - masks[k][..., None]) * st.fill_image            # blackbox.py:343
        want = np.moveaxis(masked - np.asarray(MEAN_RGB), 2, 0).astype(np.float32)                        # resnet.py:32-37
        worst = max(worst, float(np.abs(got[k] - want).max()))
        gold_sum = GOLD[case + '/masked_sums'][k]
        # float64 against float64: the reference's expression on the DEVICE's float64 masks
        total = (dev_masks[k][..., None] * st.probe + (1.0 - dev_masks[k][..., None]) * st.fill_image).sum()
        worst_sum = max(worst_sum, abs(total - gold_sum) / abs(gold_sum))
        total32 = got[k].astype(np.float64).sum() + float(np.sum(MEAN_RGB)) * 224 * 224
        worst_sum32 = max(worst_sum32, abs(total32 - gold_sum))
    REPORT['input/' + case] = {'max_abs_diff': worst, 'bar': 2.0 ** -15, 'sum_rel_err': worst_sum, 'sum_bar': 1e-9, 'fp32_sum_abs_err': worst_sum32,
                               'fp32_sum_bar': 3 * 224 * 224 * 2.0 ** -17}
    print('%s network input: max|d| = %.3e, float64 sums rel %.3e, fp32 tensor sums abs %.3e' % (case, worst, worst_sum, worst_sum32))
    assert worst <= 2.0 ** -15
    assert worst_sum <= 1e-9
    assert worst_sum32 <= 3 * 224 * 224 * 2.0 ** -17
    one = st.masked_probe(3)
    assert one.shape == (224, 224, 3) and np.abs(np.moveaxis(one, 2, 0) - (got[3].astype(np.float64) + np.asarray(MEAN_RGB)[:, None, None])).max() == 0


# ---- scores ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', MINI_CASES)
def test_scores_mini(mini48, images, case):
    st = _strise(case, images, mini48)
    st.score_masks()
    err, r = _score_error(case, st.mask_scores)
    REPORT['scores/' + case] = {'rel_err_vs_ref64': float(err), 'r_ref32_vs_ref64': float(r), 'bar': float(4 * r)}
    print('%s scores: %.3e (r = %.3e, bar %.3e)' % (case, err, r, 4 * r))
    assert st.mask_scores.shape == (48,) and st.mask_scores.dtype == np.float64
    assert err <= 4 * r
    n_refs = int(GOLD[case + '/n_refs'])
    orig = np.concatenate([st.original_probe_ref_scores.ravel(), st.original_probe_gallery_scores.ravel()])
    assert st.original_probe_ref_scores.shape == (1, n_refs)
    assert np.abs(orig - GOLD[case + '/orig64']).max() <= 1e-4


def test_scores_resnet101(gpu_device, images):
    """32 masks, one reference, one gallery image through the full-size forward (the bf16x6 path at 32 images)."""
    case = 'r101/e1'
    wb = _whitebox('stresnet101', 32, gpu_device, 65359)
    st = _strise(case, images, wb)
    st.score_masks()
    err, r = _score_error(case, st.mask_scores)
    REPORT['scores/' + case] = {'rel_err_vs_ref64': float(err), 'r_ref32_vs_ref64': float(r), 'bar': float(4 * r)}
    print('%s scores: %.3e (r = %.3e, bar %.3e)' % (case, err, r, 4 * r))
    assert err <= 4 * r
    st.compute_saliency_map(positive_scores=bool(GOLD[case + '/positive']))
    d, dist = np.abs(st.saliency_map - GOLD[case + '/map64']).max(), float(GOLD[case + '/map_dist'])
    REPORT['map_own_scores/' + case] = {'max_abs_diff': float(d), 'ref32_vs_ref64': dist, 'bar': 4 * dist}
    print('%s map from the engine\'s scores: %.3e (ref32 vs ref64 %.3e)' % (case, d, dist))
    assert d <= 4 * dist
    wb.net._engine.close()


# ---- map -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', MINI_CASES + ('r101/e1',))
def test_merge_kernel_on_the_fixtures_scores(mini48, images, case):
    """The merge alone: weights from the fixture's float64 scores, against the fixture's float64-run map."""
    eng = mini48._engine(48)
    s64 = GOLD[case + '/scores64']
    positive = bool(GOLD[case + '/positive'])
    sel = _reference_selection(s64, positive)
    sal = eng.strise_combine(np.where(sel, s64, 0.0), int(sel.sum()), GOLD[case + '/mask_cells'], GOLD[case + '/mask_shifts'], (19, 19), SCALE,
                             1 if positive else -1).cpu().numpy()
    d = np.abs(sal - GOLD[case + '/map64']).max()
    REPORT['merge/' + case] = {'max_abs_diff': float(d), 'bar': 1e-6}
    print('%s merge: max|d| = %.3e' % (case, d))
    assert sal.dtype == np.float64 and sal.min() == 0.0 and sal.max() == 1.0
    assert d <= 1e-6


@pytest.mark.parametrize('case,positive,percentile', [('mini/e1', False, 0), ('mini/e40', True, 90), ('mini/e40', False, 75), ('mini/neg', True, 0)])
def test_merge_other_branch_and_sparse_selection(mini48, case, positive, percentile):
    """The branch the fixture did not store, and selections that leave out most masks (zero weights), against blackbox.py:416-441 in numpy."""
    eng = mini48._engine(48)
    s64, cells, shifts = GOLD[case + '/scores64'], GOLD[case + '/mask_cells'], GOLD[case + '/mask_shifts']
    sel = _reference_selection(s64, positive, percentile)
    if percentile:
        assert sel.sum() <= len(s64) // 4
    want = _reference_map(s64, sel, _zoom_masks(cells, shifts, 19, 224), 1 if positive else -1)
    sal = eng.strise_combine(np.where(sel, s64, 0.0), int(sel.sum()), cells, shifts, (19, 19), SCALE, 1 if positive else -1).cpu().numpy()
    d = np.abs(sal - want).max()
    REPORT['merge_numpy/%s/%s/p%d' % (case, 'pos' if positive else 'neg', percentile)] = {'max_abs_diff': float(d), 'bar': 1e-6, 'selected': int(sel.sum())}
    print('%s %s percentile %d (%d selected): max|d| = %.3e' % (case, positive, percentile, sel.sum(), d))
    assert d <= 1e-6


@pytest.mark.parametrize('case', MINI_CASES)
def test_map_from_the_engines_own_scores(mini48, images, case):
    st = _strise(case, images, mini48)
    st.score_masks()
    positive = bool(GOLD[case + '/positive'])
    st.compute_saliency_map(positive_scores=positive)
    assert np.array_equal(st.selected_indices, _reference_selection(GOLD[case + '/scores64'], positive))
    d, dist = np.abs(st.saliency_map - GOLD[case + '/map64']).max(), float(GOLD[case + '/map_dist'])
    REPORT['map_own_scores/' + case] = {'max_abs_diff': float(d), 'ref32_vs_ref64': dist, 'bar': 4 * dist}
    print('%s map from the engine\'s scores: %.3e (ref32 vs ref64 %.3e)' % (case, d, dist))
    assert d <= 4 * dist


# ---- batching --------------------------------------------------------------------------------------------------------------------------
def test_partial_batch_is_padded_and_dropped(mini32, mini48, images):
    """48 masks + the probe = 49 images: two batches of 32 (15 all-ones paddings) or two of 48 (47); both hold the score bar."""
    case = 'mini/e1'
    for tag, wb in (('batch32', mini32), ('batch48', mini48)):
        st = _strise(case, images, wb)
        st.score_masks()
        err, r = _score_error(case, st.mask_scores)
        REPORT['scores/%s/%s' % (case, tag)] = {'rel_err_vs_ref64': float(err), 'r_ref32_vs_ref64': float(r), 'bar': float(4 * r)}
        print('%s %s scores: %.3e (bar %.3e)' % (case, tag, err, 4 * r))
        assert st.mask_scores.shape == (48,) and np.isfinite(st.mask_scores).all()
        assert err <= 4 * r
        # the unmasked probe rode along as image zero: its scores are those of a lone encode, within the forward's tolerance (1e-4 of the
        # embedding's maximum, tools/embeddings_sweep.py; the similarity is 1/2-Lipschitz in the unit vectors)
        p = wb.encode(BB.convert_resnet101v4_image(images[0]).unsqueeze(0).to(wb.net.net.device)).double().cpu().numpy()
        g = st._embed(list(images[1:4]) + list(images[4:7])).double().cpu().numpy()
        unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)      # noqa: E731
        lone = 1.0 - 0.5 * np.linalg.norm(unit(p) - unit(g), axis=1)
        orig = np.concatenate([st.original_probe_ref_scores.ravel(), st.original_probe_gallery_scores.ravel()])
        assert np.abs(orig - lone).max() <= 1e-4


def test_seven_batches_reuse_both_buffers(gpu_device, images):
    """48 masks + the probe = 49 images on an engine of 8: seven batches, so each of the two input buffers is handed back to the side stream
    (ev_free) several times; the last batch holds one real image and seven paddings."""
    case = 'mini/e1'
    st = _strise(case, images, _whitebox('stresnet_mini', 8, gpu_device, 5))
    st.score_masks()
    err, r = _score_error(case, st.mask_scores)
    REPORT['scores/%s/batch8' % case] = {'rel_err_vs_ref64': float(err), 'r_ref32_vs_ref64': float(r), 'bar': float(4 * r)}
    print('%s batch8 scores: %.3e (bar %.3e)' % (case, err, 4 * r))
    assert st.mask_scores.shape == (48,) and np.isfinite(st.mask_scores).all()
    assert err <= 4 * r


def test_single_batch_runs_no_second_generate(mini32, images):
    """The first 31 masks of the case + the probe = 32 images: exactly one batch of the engine of 32, straight through Engine.strise_score."""
    case = 'mini/e1'
    st = _strise(case, images, mini32)
    eng, enc = st._engine()
    cells, shifts, grid, scale = st._mask_args()
    scores, _ = eng.strise_score(torch.from_numpy(st.probe), torch.from_numpy(st.fill_image), cells[:31], shifts[:31], grid, scale, st._embed(st.refs),
                                 st._embed(st.gallery), enc)
    scores = scores.cpu().numpy()
    s64 = GOLD[case + '/scores64'][:31]
    err, r = np.abs(scores - s64).max() / np.abs(s64).max(), _score_error(case, GOLD[case + '/scores64'])[1]
    REPORT['scores/%s/first31' % case] = {'rel_err_vs_ref64': float(err), 'r_ref32_vs_ref64': float(r), 'bar': float(4 * r)}
    print('%s first 31 masks, one batch: %.3e (bar %.3e)' % (case, err, 4 * r))
    assert scores.shape == (31,) and np.isfinite(scores).all()
    assert err <= 4 * r


# ---- error paths -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(mini48, lcnn, images):
    eng = mini48._engine(48)
    enc = mini48.net._mark('encode')
    probe, fill = torch.from_numpy(images[0]), torch.full((224, 224, 3), 0.5, dtype=torch.float64)
    cells = np.array([[5], [7]], dtype=np.int32)
    shifts = np.array([[0, 0], [3, 4]], dtype=np.int32)
    emb = torch.ones((3, 512))
    with pytest.raises(ValueError, match='2 references against 3 gallery images'):
        eng.strise_score(probe, fill, cells, shifts, (19, 19), SCALE, emb[:2], emb, enc)
    with pytest.raises(ValueError, match='cell index 361'):
        eng.strise_score(probe, fill, np.array([[5], [361]], dtype=np.int32), shifts, (19, 19), SCALE, emb, emb, enc)
    with pytest.raises(ValueError, match=r'shift 12 of mask 1 outside \[0, 12\)'):
        eng.strise_masks(cells, np.array([[0, 0], [3, 12]], dtype=np.int32), (19, 19), SCALE)
    with pytest.raises(ValueError, match='draws cell 5 twice'):
        eng.strise_combine(np.ones(1), 1, np.array([[5, 5]], dtype=np.int32), shifts[:1], (19, 19), SCALE)
    with pytest.raises(ValueError, match='mask_scale 225 exceeds the 224 x 224 input'):
        eng.strise_combine(np.ones(2), 2, cells, shifts, (1, 1), 225)
    e1 = lcnn._engine(8)
    with pytest.raises(ValueError, match='3-channel network'):
        e1.strise_score(torch.zeros((128, 128, 3), dtype=torch.uint8), torch.zeros((128, 128, 3), dtype=torch.float64), cells, shifts, (11, 11), SCALE,
                        torch.ones((1, 256)), torch.ones((1, 256)), lcnn.net._mark('encode'))
    torch.cuda.synchronize()


# ---- the drop-in class, end to end --------------------------------------------------------------------------------------------------------
def test_evaluate_end_to_end(mini48, images):
    case = 'mini/e1'
    st = BB.STRise(probe=images[0], refs=list(images[1:4]), gallery=list(images[4:7]), black_box='resnetv4_pytorch', num_masks=48,
                   num_mask_elements=1, net=mini48)
    np.random.seed(int(GOLD[case + '/seed']))
    st.evaluate()
    assert np.abs(st.prior - BB.resize_linear(GOLD['mini/P_prior'], (224, 224))).max() <= 1e-3 * GOLD['mini/P_prior'].max()
    assert np.array_equal(st.mask_cells, GOLD[case + '/mask_cells']) and np.array_equal(st.mask_shifts, GOLD[case + '/mask_shifts']), \
        'the draws differ from the reference\'s: the prior moved a cell across the median cut or a draw across a bin edge'
    err, r = _score_error(case, st.mask_scores)
    d, dist = np.abs(st.saliency_map - GOLD[case + '/map64']).max(), float(GOLD[case + '/map_dist'])
    REPORT['evaluate/' + case] = {'scores_rel_err': float(err), 'scores_bar': float(4 * r), 'map_max_abs_diff': float(d), 'map_bar': 4 * dist}
    print('evaluate: scores %.3e (bar %.3e), map %.3e (bar %.3e)' % (err, 4 * r, d, 4 * dist))
    assert err <= 4 * r and d <= 4 * dist


def test_user_callable_black_box(mini48, images):
    """A black_box_fn that wraps the same network: the masked probes come from the device kernel, batch by batch, as arrays."""
    case = 'mini/e1'
    helper = BB.STRise(probe=images[0], refs=list(images[1:4]), black_box='resnetv4_pytorch', net=mini48)
    calls = []

    def fn(probes, gallery):
        calls.append(len(probes))
        assert isinstance(probes[0], np.ndarray) and probes[0].shape == (224, 224, 3)
        return helper.resnet_bb_fn(probes, gallery)
    st = _strise(case, images, mini48, black_box=None, black_box_fn=fn)
    st.score_masks()
    assert calls == [1, 1, 48, 48]
    err, r = _score_error(case, st.mask_scores)
    REPORT['scores_callable/' + case] = {'rel_err_vs_ref64': float(err), 'bar': float(4 * r)}
    print('callable scores: %.3e (bar %.3e)' % (err, 4 * r))
    assert st.masked_probe_ref_scores.shape == (48, 3) and err <= 4 * r
