"""Host tests of match calibration (xfr_amd/calibration.py; include/xfr_amd.h: xfr_embed_templates, xfr_pair_dists, xfr_nearest_rows): the numpy
restatements against what the REAL reference computed (tests/golden/golden_calibration.npz, make_golden_calibration.py) and against the
reference's formulas restated here, and the C-ABI boundary of the three calls.  No device is needed.

Bars:
  match_threshold   thresholds, fp and tp equal to the reference's N x T comparison (calculate_net_match_threshold.py:76-88, restated below) as
                    integers, the chosen threshold to the bit;
  goldens           calc_mate_nonmate_dists: the reference's arrays exactly (the same draws, the same float32 numpy arithmetic); the printed threshold
                    to its six decimals; the separability table exactly, booleans and float32 values; the filtered-masks CSV the script wrote;
  platt_scaling     within 1e-8 relative of sklearn's tight-tolerance fit stored in the fixture (the Newton solve agrees to 4e-11), and within the
                    recorded distance of the script's default-tolerance fit from the tight one, plus 1e-6 for its six printed decimals, of the
                    printed value."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

import calibration_inputs as C
from xfr_amd import _lib
from xfr_amd import calibration as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_calibration.npz'))
NEW_SYMBOLS = ('xfr_embed_templates', 'xfr_pair_dists', 'xfr_nearest_rows')


# ---- match_threshold ----------------------------------------------------------------------------------------------------------------------
def _reference_roc(mate_dists, nonmate_dists):
    """calculate_net_match_threshold.py:76-88 as it stands (np.float is float)."""
    thresholds = np.concatenate([mate_dists, nonmate_dists])
    thresholds.sort()
    thresholds = np.insert(thresholds, 0, 0)
    thresholds = np.around(thresholds, 4)
    thresholds = np.unique(thresholds)
    fp = np.sum(nonmate_dists[:, np.newaxis] <= thresholds[np.newaxis, :], axis=0)
    fpr = fp.astype(float) / len(nonmate_dists)
    chosen_index = np.argmin(abs(fpr - 1e-4))
    thresh = thresholds[chosen_index]
    tp = np.sum(mate_dists[:, np.newaxis] <= thresholds[np.newaxis, :], axis=0)
    tpr = tp.astype(float) / len(mate_dists)
    return thresh, thresholds, fp, tp, fpr, tpr


def _roc_inputs(kind):
    rng = np.random.RandomState(5)
    if kind in ('float32', 'float64'):
        mate, nonmate = C.synthetic_dists(np.dtype(kind))
        return mate, nonmate[:3000]
    if kind == 'zero_is_a_distance':
        mate = np.abs(rng.normal(0.5, 0.2, 50)).astype(np.float32)
        mate[7] = 0.0
        return mate, np.abs(rng.normal(1.3, 0.1, 700)).astype(np.float32)
    # duplicates: distances on a grid of 1e-4 and finer, so that many are equal and many more round to the same threshold
    return (rng.randint(2000, 9000, 80) * 1e-4).astype(np.float32), (rng.randint(90000, 150000, 900) * 1e-5).astype(np.float32)


@pytest.mark.parametrize('kind', ['float32', 'float64', 'zero_is_a_distance', 'duplicates'])
def test_match_threshold_equals_the_reference_formula(kind):
    mate, nonmate = _roc_inputs(kind)
    thresh, thresholds, fp, tp, fpr, tpr = _reference_roc(mate, nonmate)
    got_thresholds, got_fp, got_tp = K._roc_counts(mate, nonmate)
    assert got_thresholds.dtype == thresholds.dtype and np.array_equal(got_thresholds, thresholds)
    assert np.array_equal(got_fp.astype(np.int64), fp.astype(np.int64)) and np.array_equal(got_tp.astype(np.int64), tp.astype(np.int64))
    got = K.match_threshold(mate, nonmate)
    assert got[0].dtype == thresh.dtype and got[0].tobytes() == thresh.tobytes()
    assert np.array_equal(got[1], thresholds) and np.array_equal(got[2], fpr) and np.array_equal(got[3], tpr)
    if kind == 'duplicates':
        assert len(np.unique(np.concatenate([mate, nonmate]))) < mate.size + nonmate.size and thresholds.size < len(np.unique(nonmate)) + mate.size
    if kind == 'zero_is_a_distance':
        assert thresholds[0] == 0 and thresholds[1] > 0 and tp[0] == 1


def test_match_threshold_takes_the_fmr():
    mate, nonmate = C.synthetic_dists()
    loose, strict = K.match_threshold(mate, nonmate, fmr=1e-2)[0], K.match_threshold(mate, nonmate, fmr=1e-4)[0]
    assert loose > strict
    assert abs((nonmate <= loose).mean() - 1e-2) < 1e-3


# ---- the goldens --------------------------------------------------------------------------------------------------------------------------
def test_calc_mate_nonmate_dists_reproduces_the_reference(tmp_path):
    import shutil
    os.makedirs(tmp_path / 'protocols')
    shutil.copy(os.path.join(ROOT, 'tests', 'golden', C.METADATA_CSV), tmp_path / 'protocols' / 'ijbc_metadata.csv')
    mate, nonmate = K.calc_mate_nonmate_dists(C.MetadataNet(), C.CALIB_SUBJECTS, C.CALIB_SEED, str(tmp_path / 'out'), str(tmp_path))
    assert mate.dtype == np.float32 and nonmate.dtype == np.float32
    assert mate.shape == GOLD['calib/mate_dists'].shape and nonmate.shape == (mate.size * 2 * 64,)
    assert np.array_equal(mate, GOLD['calib/mate_dists']) and np.array_equal(nonmate, GOLD['calib/nonmate_dists'])
    assert os.path.isdir(tmp_path / 'out')                                                       # :84


def test_committed_metadata_is_the_generated_table(tmp_path):
    C.write_metadata(tmp_path / 'm.csv')
    assert open(tmp_path / 'm.csv').read() == open(os.path.join(ROOT, 'tests', 'golden', C.METADATA_CSV)).read()


def test_threshold_reproduces_the_script():
    mate, nonmate = GOLD['thr/mate_dists'], GOLD['thr/nonmate_dists']
    thresh = K.match_threshold(mate, nonmate)[0]
    assert '%f' % thresh == '%f' % float(GOLD['thr/printed_thresh'])


def test_platt_scaling_against_sklearn_and_the_script():
    mate, nonmate = GOLD['thr/mate_dists'], GOLD['thr/nonmate_dists']
    thresh = K.match_threshold(mate, nonmate)[0]
    alpha = K.platt_scaling(mate, nonmate, thresh)
    tight, printed, apart = float(GOLD['thr/alpha_tight']), float(GOLD['thr/printed_alpha']), float(GOLD['thr/script_to_tight'])
    print('platt scaling %.12f, sklearn tight %.12f (%.2e relative apart), the script printed %.6f (its fit is %.2e from the tight one)' %
          (alpha, tight, abs(alpha - tight) / abs(tight), printed, apart))
    assert abs(alpha - tight) <= 1e-8 * abs(tight)
    assert abs(alpha - printed) <= apart * abs(tight) + 1e-6


def test_platt_scaling_minimises_the_objective():
    """Its own check, on float64 distances: the derivative of sklearn's objective vanishes at alpha and the objective is no lower on either side."""
    mate, nonmate = C.synthetic_dists(np.float64)
    x = np.concatenate([mate, nonmate]) - 1.05
    s = np.where(np.arange(x.size) < mate.size, -x, x)
    alpha = K.platt_scaling(mate, nonmate, 1.05)
    f = lambda w: 0.5 * w * w + np.logaddexp(0.0, -s * w).sum()
    grad = alpha - (s / (1.0 + np.exp(s * alpha))).sum()
    assert abs(grad) < 1e-9 * (1.0 + np.abs(s).sum())
    assert f(alpha) <= f(alpha * (1 + 1e-4)) and f(alpha) <= f(alpha * (1 - 1e-4))


def test_calibrate_sets_the_whitebox_attributes():
    class Net(object):
        match_threshold = platts_scaling = None
    wb = Net()
    mate, nonmate = GOLD['thr/mate_dists'], GOLD['thr/nonmate_dists']
    thresh, alpha = K.calibrate(wb, mate, nonmate)
    assert (wb.match_threshold, wb.platts_scaling) == (thresh, alpha) and isinstance(thresh, float) and isinstance(alpha, float)
    assert '%f' % thresh == '%f' % float(GOLD['thr/printed_thresh']) and abs(alpha - float(GOLD['thr/alpha_tight'])) <= 1e-8 * alpha


@pytest.fixture(scope='module')
def game(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('game'))
    C.write_game_tree(root)
    table, subjects = K.separability_table(C.GameNet(), root, net_name=C.NET_NAME, return_subject_data=True)
    return table, subjects


def test_separability_table_reproduces_the_script(game):
    table, _ = game
    assert list(table.columns) == K.SEPARABILITY_COLUMNS and len(K.SEPARABILITY_COLUMNS) == 13
    got = C.table_arrays(table)
    for column in K.SEPARABILITY_COLUMNS:
        want = GOLD['sep/' + column]
        assert got[column].dtype == want.dtype and np.array_equal(got[column], want), column
    assert got['OrigTripletSim'].dtype == np.float32 and got['CorrectlyCls'].dtype == bool


def test_triplet_separability_is_one_cell_of_the_table(game, tmp_path):
    table, _ = game
    root = str(tmp_path)
    sid, mask = 8, 5
    probes, refs = C.SUBJECTS[sid]
    name = lambda pattern, fn, **kw: os.path.join(root, pattern.format(SUBJECT_ID=sid, ORIGINAL_BASENAME=os.path.splitext(fn)[0], **kw))
    got = K.triplet_separability(C.GameNet(), [name(K.ORIGINAL_PATTERN_REL, fn) for fn in probes], [name(K.ORIGINAL_PATTERN_REL, fn) for fn in refs],
                                 [name(K.INPAINTING_PATTERN_REL, fn, MASK_ID=mask) for fn in probes],
                                 [name(K.INPAINTING_PATTERN_REL, fn, MASK_ID=mask) for fn in refs])
    rows = table[(table['SUBJECT_ID'] == sid) & (table['MASK_ID'] == mask)]
    for cells, column in zip(got, ('CorrectlyCls', 'OrigTripletSim', 'TwinCorrectlyCls', 'TwinTripletSim')):
        assert cells.shape == (len(probes), 1)
        assert np.array_equal(cells[:, 0], np.array([v[0] for v in rows[column]]))


def test_include_masks_by_thresholds_reproduces_the_script(game):
    import pandas as pd
    assert bool(GOLD['sep/tail_ran'])
    table, subjects = game
    got = K.include_masks_by_thresholds(table, subjects)
    want = pd.read_csv(io.StringIO(str(GOLD['sep/filtered_csv'])))
    text = io.StringIO()
    got.to_csv(text, index=False)
    got = pd.read_csv(io.StringIO(text.getvalue()))
    key = ['SUBJECT_ID', 'MASK_ID', 'TRIPLET_SET', 'ORIGINAL_BASENAME']
    pd.testing.assert_frame_equal(got.sort_values(key).reset_index(drop=True), want.sort_values(key).reset_index(drop=True))


def test_include_masks_by_thresholds_on_a_hand_made_table():
    import pandas as pd
    cell = lambda v: np.array([v])
    rows = []
    for sid, mask, fn, ok, twin_ok in [(1, 0, 'a', True, True), (1, 0, 'b', True, False), (1, 2, 'a', False, True), (1, 2, 'b', True, False),
                                       (2, 0, 'c', True, True)]:
        rows.append(('resnet', sid, fn + '.jpg', fn, 'PROBE', mask, cell(ok), cell(np.float32(0.25)), cell(twin_ok), cell(np.float32(0.5)),
                     K.ORIGINAL_PATTERN_REL.format(SUBJECT_ID=sid, ORIGINAL_BASENAME=fn),
                     K.INPAINTING_PATTERN_REL.format(SUBJECT_ID=sid, ORIGINAL_BASENAME=fn, MASK_ID=mask), 'average'))
    table = pd.DataFrame(rows, columns=K.SEPARABILITY_COLUMNS)
    subjects = pd.DataFrame([(1, 'a.jpg', 'PROBE', 'a'), (1, 'b.jpg', 'PROBE', 'b'), (1, 'r.jpg', 'REF', 'r'), (1, 's.jpg', 'REF', 's'),
                             (2, 'c.jpg', 'PROBE', 'c'), (2, 't.jpg', 'REF', 't')], columns=['SUBJECT_ID', 'ORIGINAL_FILE', 'TRIPLET_SET', 'ORIGINAL_BASENAME'])
    got = K.include_masks_by_thresholds(table, subjects)
    # subject 1 keeps probe a under mask 0 and its two references; mask 2 keeps nothing; subject 2 keeps probe c and its reference
    assert [tuple(r) for r in got[['SUBJECT_ID', 'MASK_ID', 'ORIGINAL_BASENAME', 'TRIPLET_SET']].values] == [
        (1, 0, 'a', 'PROBE'), (1, 0, 'r', 'REF'), (1, 0, 's', 'REF'), (2, 0, 'c', 'PROBE'), (2, 0, 't', 'REF')]
    assert list(got.columns) == ['SUBJECT_ID', 'MASK_ID', 'ORIGINAL_BASENAME', 'OriginalFile', 'InpaintingFile', 'TRIPLET_SET', 'OrigTripletSim_resnet',
                                 'TwinTripletSim_resnet']
    probes = got[got['TRIPLET_SET'] == 'PROBE']
    assert (probes['OrigTripletSim_resnet'] == np.float32(0.25)).all() and (probes['TwinTripletSim_resnet'] == np.float32(0.5)).all()
    assert got[got['TRIPLET_SET'] == 'REF']['OrigTripletSim_resnet'].isna().all()
    assert got.iloc[1]['InpaintingFile'] == 'aligned/1/r/inpainted/00000_out_0.png'


def test_nearest_nonmates_host_restatement():
    """eccv20.py:53-59 on a stub whose net.encode is the identity on 2 x DIM chunks."""
    import torch
    from scipy.spatial.distance import pdist, squareform

    class Net(object):
        def encode(self, x):
            return x

    class Wb(object):
        net = Net()
    rng = np.random.RandomState(2)
    chunks = [torch.from_numpy(rng.randn(2, C.DIM).astype(np.float32)) for _ in range(7)]
    ids = ['n%06d' % i for i in range(7)]
    got = K.nearest_nonmates(Wb(), chunks, ids, 3)
    X = np.array([c.sum(dim=0).numpy() for c in chunks])
    X = X / np.linalg.norm(X, axis=1, keepdims=True)
    for k, d in enumerate(squareform(pdist(X, metric='euclidean'))):
        assert got[ids[k]] == [ids[j] for j in np.argsort(d)[1:][0:3]]
        assert ids[k] not in got[ids[k]]


# ---- the C-ABI boundary -------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_new_symbols():
    src = open(os.path.join(ROOT, 'include', 'xfr_amd.h')).read()
    assert re.search(r'#define XFR_AMD_ABI_VERSION 7\b', src) and _lib.ABI_VERSION == 7
    lib = _lib.load()
    assert lib.xfr_abi_version() == 7
    bound = dict((n, a) for n, _, a in _lib.SYMBOLS)
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in NEW_SYMBOLS:
        decl = re.search(r'xfr_status XFR_EX %s\((.*?)\);' % name, code, flags=re.S)
        assert decl, name
        assert len(decl.group(1).split(',')) == len(bound[name]), name
        assert hasattr(lib, name)
        assert not name.startswith('xfr_inpaint_') and not name.startswith('xfr_strise_')
    assert int(re.search(r'#define XFR_MATCH_MAX_K (\d+)', src).group(1)) == _lib.MATCH_MAX_K == 64
    assert int(re.search(r'#define XFR_MATCH_MAX_D (\d+)', src).group(1)) == _lib.MATCH_MAX_D == 4096
    for name in NEW_SYMBOLS:      # each declaration cites the reference lines it replaces
        comment = src[:src.index('xfr_status XFR_EX %s(' % name)].rsplit('/*', 1)[1]
        assert re.search(r'\.py:\d+', comment), name


def test_argument_checks_that_need_no_device():
    lib = _lib.load()
    rows, offsets, pairs = (ctypes.c_int32 * 2)(0, 1), (ctypes.c_int32 * 2)(0, 2), (ctypes.c_int32 * 2)(0, 0)
    p = ctypes.c_void_p(64)      # never dereferenced: the engine is refused first
    for call in (lambda: lib.xfr_embed_templates(None, p, 2, 8, rows, offsets, 1, 1, p, None),
                 lambda: lib.xfr_pair_dists(None, p, 2, p, 2, 8, pairs, 1, p, None),
                 lambda: lib.xfr_nearest_rows(None, p, 2, p, 2, 8, 1, 0, p, p, None)):
        assert call() == _lib.XFR_INVALID_ARG
        assert b'null engine' in lib.xfr_last_error()
        with pytest.raises(ValueError, match='null engine'):
            _lib.check(call())
