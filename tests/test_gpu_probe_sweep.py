"""GPU tests of the sweep state that STRise and inpainting-game scoring share on one engine (csrc/probe_sweep.hip: side stream, events, the two input
buffers, the embedding buffer): calls of the two families interleaved without a synchronisation, on one stream and on two.  Every result is held
to the bar of its own family's tests (tests/test_gpu_strise.py, tests/test_gpu_inpaint_game.py): 4 r on scores and distances, r read from the
fixtures, no classification flip, IoU counts and the merge of the fixture's scores as there.  Plain parity tests: each runs once."""
import numpy as np
import pytest
import torch

import inpaint_game_inputs as I
import probe_scoring_utils as U
from probe_scoring_utils import images, mini32      # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
SGOLD, IGOLD = U.gold('strise'), U.gold('inpaint_game')
SCASE, ICASE, SCALE = 'mini/e1', 'mini/zero_on', 12


def _strise_score(st):
    """Engine.strise_score of the case's 48 masks; the scores stay on the device."""
    eng, enc = st._engine()
    cells, shifts, grid, scale = st._mask_args()
    return eng.strise_score(torch.from_numpy(st.probe), torch.from_numpy(st.fill_image), cells, shifts, grid, scale, st._embed(st.refs),
                            st._embed(st.gallery), enc)[0]


def _inpaint_score(wb):
    """Engine.inpaint_score of the case; cls, pg, pr stay on the device."""
    c = U.inpaint_case(IGOLD, ICASE)
    a, b = I.probe_pair(c['arch'])
    return wb._engine(wb.batch_size).inpaint_score(c['maps'], c['levels'], a, b, IGOLD['mini/gal_orig'], IGOLD['mini/gal_inp'], wb.net._mark('encode'),
                                                   method=c['method'], noise=c['noise'], include_zero=c['include_zero'])


def _check_strise(tag, scores):
    scores = scores.cpu().numpy()
    err, r = U.score_error(SGOLD, SCASE, scores)
    print('%s STRise scores: %.3e (bar %.3e)' % (tag, err, 4 * r))
    assert scores.shape == (48,) and np.isfinite(scores).all()
    assert err <= 4 * r


def _check_inpaint(tag, got):
    cls, pg, pr = got
    U.check_scores(IGOLD, ICASE, tag, cls.cpu().numpy().astype(bool), pg.cpu().numpy(), pr.cpu().numpy())


def test_the_two_families_interleaved_on_one_engine(mini32, images):
    """strise_score, inpaint_score, strise_combine, inpaint_iou, strise_score, inpaint_score with no synchronisation in between: the padding and
    the leftovers of one family must not reach the other through the shared buffers."""
    st = U.strise(SGOLD, SCASE, images, mini32)
    eng = mini32._engine(32)
    c = U.inpaint_case(IGOLD, ICASE)
    s64, positive = SGOLD[SCASE + '/scores64'], bool(SGOLD[SCASE + '/positive'])
    sel = U.reference_selection(s64, positive)
    scores1 = _strise_score(st)
    game1 = _inpaint_score(mini32)
    sal = eng.strise_combine(np.where(sel, s64, 0.0), int(sel.sum()), SGOLD[SCASE + '/mask_cells'], SGOLD[SCASE + '/mask_shifts'], (19, 19), SCALE,
                             1 if positive else -1)
    iou = eng.inpaint_iou(c['maps'], c['levels'], I.ground_truth(c['arch']), method=c['method'], noise=c['noise'], include_zero=c['include_zero'])
    scores2 = _strise_score(st)
    game2 = _inpaint_score(mini32)
    _check_strise('first', scores1)
    _check_inpaint('/shared_first', game1)
    assert np.abs(sal.cpu().numpy() - SGOLD[SCASE + '/map64']).max() <= 1e-6
    assert np.array_equal(iou.cpu().numpy(), IGOLD[ICASE + '/iou_counts'])
    _check_strise('second', scores2)
    _check_inpaint('/shared_second', game2)


def test_the_two_families_from_two_streams(mini32, images, gpu_device):
    """strise_score under one stream, inpaint_score under another, one device synchronisation at the end: the calls of one engine are ordered one
    behind another whatever streams they are given (include/xfr_amd.h), so both hold their bars."""
    st = U.strise(SGOLD, SCASE, images, mini32)
    s1, s2 = torch.cuda.Stream(gpu_device), torch.cuda.Stream(gpu_device)
    with torch.cuda.stream(s1):
        scores = _strise_score(st)
    with torch.cuda.stream(s2):
        game = _inpaint_score(mini32)
    torch.cuda.synchronize()
    _check_strise('stream 1', scores)
    _check_inpaint('/two_streams', game)
