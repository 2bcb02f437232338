#!/usr/bin/env python
"""Golden values for match calibration (xfr_amd/calibration.py), produced by the REAL reference code on the CPU.
Usage: python tests/golden/make_golden_calibration.py  ->  tests/golden/golden_calibration.npz, tests/golden/calibration_ijbc_metadata.csv

Inputs are tests/calibration_inputs.py: seeded stub networks whose embeddings are a function of the file name, so the reference's stages run
without images or weights and only results (and the small metadata table) are stored.  Everything written is data.

  calib/mate_dists, calib/nonmate_dists     python/xfr/inpainting_game/net_mate_nonmate_dists.py calc_mate_nonmate_dists itself, imported through
                                            ref_import's shims (dill, pytz, matplotlib's mpl_toolkits and skimage.morphology are stubbed where absent),
                                            on the metadata table with seed CALIB_SEED and CALIB_SUBJECTS subjects.
  thr/...                                   eval/calculate_net_match_threshold.py under runpy, with an `xfr` module that points at a temporary directory
                                            holding one dists_*.npz of calibration_inputs.synthetic_dists(); np.float and np.int (:83,:94), removed
                                            from numpy 1.24, are this file's shims.  printed_thresh, printed_alpha: parsed from its output (six
                                            decimals).  alpha_tight: LogisticRegression(fit_intercept=False, tol=1e-12, max_iter=10000) on the same
                                            data; script_to_tight: |alpha of the script's default-tolerance fit - alpha_tight| / |alpha_tight|.
  sep/<column>                              eval/filter_inpaintinggame_for_net.py under runpy, with stubbed `create_wbnet` and `xfr` modules and the
                                            two-subject tree of calibration_inputs.write_game_tree: its `separability` table, rows ordered by
                                            (subject, mask, file).  sep/tail_ran says whether the script's tail (include_masks_by_thresholds, :261-352)
                                            ran under this pandas; where it did, sep/filtered_csv holds the CSV it wrote; where it did not, the table
                                            was taken from the failing frame's globals and include_masks_by_thresholds is pinned by a hand-made table
                                            only (tests/test_calibration_host.py)."""
import contextlib
import glob
import io
import os
import re
import runpy
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402
import calibration_inputs as C  # noqa: E402

import matplotlib  # noqa: E402
matplotlib.use('Agg')
for _name in ('float', 'int', 'bool'):
    if not hasattr(np, _name):
        setattr(np, _name, {'float': float, 'int': int, 'bool': bool}[_name])


def stub_missing(*names):
    for name in names:
        try:
            __import__(name)
        except ImportError:
            parts = name.split('.')
            for i in range(1, len(parts) + 1):
                sys.modules.setdefault('.'.join(parts[:i]), types.ModuleType('.'.join(parts[:i])))


def xfr_stub(game_dir, root):
    m = types.ModuleType('xfr')
    m.inpaintgame2_dir, m.xfr_root, m.inpaintgame_saliencymaps_dir = game_dir, root, os.path.join(root, 'saliency')
    return m


@contextlib.contextmanager
def script_environment(argv, **modules):
    saved_argv, saved = sys.argv, {k: sys.modules.get(k) for k in modules}
    sys.argv = argv
    sys.modules.update(modules)
    try:
        yield
    finally:
        sys.argv = saved_argv
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def calibration_distances(out):
    ref_import._install_shims()
    stub_missing('dill', 'pytz', 'imageio', 'skimage.morphology', 'skimage.transform', 'skimage.filters')
    sys.path.insert(0, os.path.join(ref_import.REF_ROOT, 'python'))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        from xfr.inpainting_game.net_mate_nonmate_dists import calc_mate_nonmate_dists
    C.write_metadata(os.path.join(HERE, C.METADATA_CSV))
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'protocols'))
        C.write_metadata(os.path.join(tmp, 'protocols', 'ijbc_metadata.csv'))
        with contextlib.redirect_stdout(io.StringIO()):
            mate, nonmate = calc_mate_nonmate_dists(C.MetadataNet(), C.CALIB_SUBJECTS, C.CALIB_SEED, os.path.join(tmp, 'out'), tmp)
    assert mate.dtype == np.float32 and nonmate.dtype == np.float32 and nonmate.size == mate.size * 2 * 64
    assert mate.size < C.CALIB_SUBJECTS, 'the draw must include the subject with a single usable row'
    print('calibration distances: %d subjects, mates %.3f..%.3f, non-mates %.3f..%.3f' % (mate.size, mate.min(), mate.max(), nonmate.min(), nonmate.max()))
    out['calib/mate_dists'], out['calib/nonmate_dists'] = mate, nonmate


def threshold_and_platt(out):
    from sklearn.linear_model import LogisticRegression
    mate, nonmate = C.synthetic_dists()
    with tempfile.TemporaryDirectory() as tmp:
        in_dir = os.path.join(tmp, 'output', 'ROC_Curve_Analysis_Inpainting_Game/Net=%s' % C.NET_NAME)
        os.makedirs(in_dir)
        np.savez_compressed(os.path.join(in_dir, 'dists_net=%s_seed=1.npz' % C.NET_NAME), mate_dists=mate, nonmate_dists=nonmate)
        text = io.StringIO()
        with script_environment(['calculate_net_match_threshold.py', C.NET_NAME], xfr=xfr_stub(os.path.join(tmp, 'game'), tmp)), \
                contextlib.redirect_stdout(text):
            os.environ.setdefault('IJBC_PATH', tmp)
            runpy.run_path(os.path.join(ref_import.REF_ROOT, 'eval', 'calculate_net_match_threshold.py'), run_name='__main__')
    thresh = float(re.search(r'wb\.match_threshold = ([0-9.eE+-]+)', text.getvalue()).group(1))
    alpha = float(re.search(r'wb\.platts_scaling = ([0-9.eE+-]+)', text.getvalue()).group(1))
    x = (np.concatenate([mate, nonmate]) - np.float32(thresh))[:, np.newaxis]
    y = np.ones(x.shape[0], dtype=int)
    y[:mate.size] = 0

    def fit(**kw):
        return float(LogisticRegression(fit_intercept=False, **kw).fit(x, y).coef_[0, 0])
    tight, loose = fit(tol=1e-12, max_iter=10000), fit()
    print('threshold %.6f, printed alpha %.6f, default-tolerance fit %.9f, tight fit %.12f (%.2e relative apart)' %
          (thresh, alpha, loose, tight, abs(loose - tight) / abs(tight)))
    assert abs(loose - alpha) <= 1e-6
    out.update({'thr/mate_dists': mate, 'thr/nonmate_dists': nonmate, 'thr/printed_thresh': thresh, 'thr/printed_alpha': alpha,
                'thr/alpha_tight': tight, 'thr/script_to_tight': abs(loose - tight) / abs(tight)})


def separability(out):
    cw = types.ModuleType('create_wbnet')
    cw.create_wbnet = lambda net_name, device=None: C.GameNet()
    script = os.path.join(ref_import.REF_ROOT, 'eval', 'filter_inpaintinggame_for_net.py')
    with tempfile.TemporaryDirectory() as tmp:
        game = os.path.join(tmp, 'game')
        C.write_game_tree(game)
        tail_ran, csv_text = True, ''
        with script_environment(['filter_inpaintinggame_for_net.py', C.NET_NAME], xfr=xfr_stub(game, tmp), create_wbnet=cw), \
                contextlib.redirect_stdout(io.StringIO()):
            try:
                g = runpy.run_path(script, run_name='__main__')
            except Exception as err:
                tail_ran = False
                tb = err.__traceback__
                while tb is not None:
                    if tb.tb_frame.f_code.co_filename == script and 'separability' in tb.tb_frame.f_globals:
                        g = tb.tb_frame.f_globals
                    tb = tb.tb_next
                failure = '%s: %s' % (type(err).__name__, err)
        if tail_ran:
            written = glob.glob(os.path.join(game, 'filtered_masks_threshold-*.csv'))
            assert len(written) == 1, written
            csv_text = open(written[0]).read()
    table = g['separability']
    assert list(table.columns) == ['NET', 'SUBJECT_ID', 'ORIGINAL_FILE', 'ORIGINAL_BASENAME', 'TRIPLET_SET', 'MASK_ID', 'CorrectlyCls', 'OrigTripletSim',
                                   'TwinCorrectlyCls', 'TwinTripletSim', 'OriginalFile', 'InpaintingFile', 'BestGalleryFile']
    arrays = C.table_arrays(table)
    both = arrays['CorrectlyCls'] & arrays['TwinCorrectlyCls']
    print('separability: %d rows, %d originals and %d twins correct, %d both; the tail %s' %
          (len(table), arrays['CorrectlyCls'].sum(), arrays['TwinCorrectlyCls'].sum(), both.sum(), 'ran' if tail_ran else 'failed (%s)' % failure))
    assert 0 < both.sum() < len(table), 'the tree must hold separable and inseparable triplets'
    for k, v in arrays.items():
        out['sep/' + k] = v
    out['sep/tail_ran'] = tail_ran
    out['sep/filtered_csv'] = csv_text
    return arrays


def main():
    assert ref_import.available(), 'the reference checkout is needed to make fixtures'
    out = {}
    calibration_distances(out)
    threshold_and_platt(out)
    separability(out)
    path = os.path.join(HERE, 'golden_calibration.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
