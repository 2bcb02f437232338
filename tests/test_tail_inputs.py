"""The inputs and the truth of tests/test_gpu_contrast_tail.py, proven without a device: every precondition under which that file may demand
equality to the bit is a property of tests/tail_inputs.py alone and is asserted here, so that no GPU case needs a run-time skip or a relaxed bar.
  * the generators: float32, non-negative, every sample total positive, no non-zero quotient below 2^-100, every row of a call with its own total
  * gap >= 1e-7 at every percentile strictly between 0 and 100: the cumulative sum passes the target at a distance no float64 summation order
    and no float32 / float64 reading of pct / 100 can bridge, so the cut INDEX is decided by the inputs
  * sum_margin >= 1e-9: no sample sum lies near a float32 rounding boundary, so float32(S) is decided by the inputs
  * the truth itself against the reference's lines (whitebox.py:550-556) restated in float64, and against a case small enough to do by hand."""
import numpy as np
import pytest

import tail_inputs as T

CASES = [(f, s) for f in T.FAMILIES for s in T.SHAPES]
IDS = ['%s-%dx%dx%d' % ((f,) + s) for f, s in CASES]


def test_truth_on_a_case_done_by_hand():
    P = np.array([[[1, 2, 3, 4], [4, 3, 2, 1]]], dtype=np.float32)      # C = 1, N = 1, HW = 4; both sums are 10
    f = np.float32
    t = T.truth(P, 1, 50.0)      # cumulative sums .1 .3 .6 1: the target .5 is first reached at .3
    assert t.S64.tolist() == [10.0, 10.0]
    assert t.thr[0] == f(3) / f(10)
    assert np.array_equal(t.out[0], np.array([0, 0, f(3) / f(10) - f(2) / f(10), f(4) / f(10) - f(1) / f(10)], dtype=f))
    assert abs(t.gap[0] - 0.1) < 1e-7
    t = T.truth(P, 1, None)      # no mask: the first two differences are negative and clamp to 0 all the same
    assert t.thr is None and np.array_equal(t.out[0], T.truth(P, 1, 50.0).out[0])
    assert T.truth(P, 1, 0.0).thr[0] == f(1) / f(10) and T.truth(P, 1, 100.0).thr[0] == f(4) / f(10)
    P = np.array([[[2, 2, 1, 2], [1, 1, 1, 1]]], dtype=np.float32)      # ties of the cut value are all kept
    t = T.truth(P, 1, 50.0)
    assert t.thr[0] == f(2) / f(7) and np.count_nonzero(t.out[0]) == 3


@pytest.mark.parametrize('family,shape', CASES, ids=IDS)
def test_generators(family, shape):
    C, N, HW = shape
    P = T.case(family, shape)
    assert P.dtype == np.float32 and P.shape == (C, 2 * N, HW) and not P.flags.writeable
    assert np.array_equal(P, T.make_P(family, shape)), 'seeded'
    assert np.isfinite(P).all() and (P >= 0).all()
    t = T.case_truth(family, shape, None)
    assert (t.S64 > 0).all()
    assert t.m[t.m > 0].min() >= 2.0 ** -100
    S = np.sort(t.S64)
    assert (np.diff(S) > 1e-3 * S[1:]).all(), 'every row of a call has a total of its own: %s' % (t.S64,)
    assert P.nbytes <= 2 * 2 ** 20 + 2 ** 17


@pytest.mark.parametrize('family,shape', CASES, ids=IDS)
def test_margins_hold_for_every_case_and_percentile(family, shape):
    for pct in T.PERCENTILES:
        t = T.case_truth(family, shape, pct)
        assert t.sum_margin.min() >= T.SUM_MARGIN_MIN, (pct, t.sum_margin)
        if 0 < pct < 100:
            assert t.gap.min() >= T.GAP_MIN, (pct, t.gap)
    assert T.case_truth(family, shape, None).sum_margin.min() >= T.SUM_MARGIN_MIN


@pytest.mark.parametrize('family,shape', CASES, ids=IDS)
def test_truth_against_the_reference_lines(family, shape):
    """The kept mask of the truth, m >= v*, equals whitebox.py:550-554 (sort, cumsum, mask scattered back; float64) everywhere except on elements
    equal to v*, of which the reference keeps the later ones of its sort and the library all; where no such element is dropped by the reference the
    contrast is the reference's :556-557 in float64.  The float32 contrast stays within (C + 1) 2^-24 of the float64 one."""
    C, N, HW = shape
    for pct in T.PERCENTILES:
        t = T.case_truth(family, shape, pct)
        for n in range(N):
            m, q = t.m[:, n, :], t.m[:, N + n, :]
            if pct in (0, 100):
                assert t.thr[n] == (m.min() if pct == 0 else m.max())
            keep, ref = m >= t.thr[n], T.reference_mask(m, pct)
            differ = keep != ref
            assert (m[differ] == t.thr[n]).all() and not (ref & ~keep).any(), (pct, n)
            assert keep[m == t.thr[n]].all() and keep.any()
            m64, q64 = m.astype(np.float64), q.astype(np.float64)
            want = np.maximum(ref * m64 - ref * q64, 0).sum(axis=0)
            clean = ~differ.any(axis=0)
            # m - q in float32 against float64: one rounding of a difference no larger than its operands
            assert np.abs(t.out64[n] - want)[clean].max(initial=0.0) <= C * 2.0 ** -24 * max(m64.max(), q64.max())
        assert (np.abs(t.out.astype(np.float64) - t.out64) <= (C + 1) * 2.0 ** -24 * t.out64).all()
    t = T.case_truth(family, shape, None)
    assert t.thr is None and np.isinf(t.gap).all()
    full = T.case_truth(family, shape, 0.0)      # at 0 the mask keeps everything: the contrastive form, to the bit
    assert np.array_equal(t.out.view(np.uint32), full.out.view(np.uint32))
