"""GPU tests of the sweep state that STRise and inpainting-game scoring share on one engine (csrc/probe_sweep.hip: side stream, events, the two input
buffers, the embedding buffer): calls of the two families interleaved without a synchronisation, on one stream and on two.  Every result is held
to the bar of its own family's tests (tests/test_gpu_strise.py, tests/test_gpu_inpaint_game.py): 4 r on scores and distances, r read from the
fixtures, no classification flip, IoU counts and the merge of the fixture's scores as there.  Plain parity tests: each runs once."""
import numpy as np
import pytest
import torch

import inpaint_game_inputs as I
import test_gpu_inpaint_game as TI
import test_gpu_strise as TS

pytestmark = pytest.mark.gpu
images = TS.images
mini32 = TS.mini32
SCASE, ICASE = 'mini/e1', 'mini/zero_on'


def _strise_score(st):
    """Engine.strise_score of the case's 48 masks; the scores stay on the device."""
    eng, enc = st._engine()
    cells, shifts, grid, scale = st._mask_args()
    return eng.strise_score(torch.from_numpy(st.probe), torch.from_numpy(st.fill_image), cells, shifts, grid, scale, st._embed(st.refs),
                            st._embed(st.gallery), enc)[0]


def _inpaint_score(wb):
    """Engine.inpaint_score of the case; cls, pg, pr stay on the device."""
    c = TI._case(ICASE)
    a, b = I.probe_pair(c['arch'])
    return wb._engine(wb.batch_size).inpaint_score(c['maps'], c['levels'], a, b, TI.GOLD['mini/gal_orig'], TI.GOLD['mini/gal_inp'], wb.net._mark('encode'),
                                                   method=c['method'], noise=c['noise'], include_zero=c['include_zero'])


def _check_strise(tag, scores):
    scores = scores.cpu().numpy()
    err, r = TS._score_error(SCASE, scores)
    print('%s STRise scores: %.3e (bar %.3e)' % (tag, err, 4 * r))
    assert scores.shape == (48,) and np.isfinite(scores).all()
    assert err <= 4 * r


def _check_inpaint(tag, got):
    cls, pg, pr = got
    TI._check_scores(ICASE, tag, cls.cpu().numpy().astype(bool), pg.cpu().numpy(), pr.cpu().numpy())


def test_the_two_families_interleaved_on_one_engine(mini32, images):
    """strise_score, inpaint_score, strise_combine, inpaint_iou, strise_score, inpaint_score with no synchronisation in between: the padding and
    the leftovers of one family must not reach the other through the shared buffers."""
    st = TS._strise(SCASE, images, mini32)
    eng = mini32._engine(32)
    c = TI._case(ICASE)
    s64, positive = TS.GOLD[SCASE + '/scores64'], bool(TS.GOLD[SCASE + '/positive'])
    sel = TS._reference_selection(s64, positive)
    scores1 = _strise_score(st)
    game1 = _inpaint_score(mini32)
    sal = eng.strise_combine(np.where(sel, s64, 0.0), int(sel.sum()), TS.GOLD[SCASE + '/mask_cells'], TS.GOLD[SCASE + '/mask_shifts'], (19, 19), TS.SCALE,
                             1 if positive else -1)
    iou = eng.inpaint_iou(c['maps'], c['levels'], I.ground_truth(c['arch']), method=c['method'], noise=c['noise'], include_zero=c['include_zero'])
    scores2 = _strise_score(st)
    game2 = _inpaint_score(mini32)
    _check_strise('first', scores1)
    _check_inpaint('/shared_first', game1)
    assert np.abs(sal.cpu().numpy() - TS.GOLD[SCASE + '/map64']).max() <= 1e-6
    assert np.array_equal(iou.cpu().numpy(), TI.GOLD[ICASE + '/iou_counts'])
    _check_strise('second', scores2)
    _check_inpaint('/shared_second', game2)


def test_the_two_families_from_two_streams(mini32, images, gpu_device):
    """strise_score under one stream, inpaint_score under another, one device synchronisation at the end: the calls of one engine are ordered one
    behind another whatever streams they are given (include/xfr_amd.h), so both hold their bars."""
    st = TS._strise(SCASE, images, mini32)
    s1, s2 = torch.cuda.Stream(gpu_device), torch.cuda.Stream(gpu_device)
    with torch.cuda.stream(s1):
        scores = _strise_score(st)
    with torch.cuda.stream(s2):
        game = _inpaint_score(mini32)
    torch.cuda.synchronize()
    _check_strise('stream 1', scores)
    _check_inpaint('/two_streams', game)
