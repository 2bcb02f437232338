"""The tail of truncated_contrastive_ebp held to an exact truth: sample_sums_kernel, the 4-pass radix select (trunc_hist_kernel /
trunc_select_kernel) and contrast_kernel of xfr_amd/csrc/saliency.hip, run by xfr_debug_contrast_tail on inputs of tests/tail_inputs.py, against
tail_inputs.truth: the sums to their float32 rounding and 1e-12, the threshold and the contrast TO THE BIT.  The decision the tail makes is
discrete -- which elements of m = P / S survive -- and the two older tests of it (test_truncation_tail_equals_reference_formula_on_engine_P,
test_truncated_contrastive_tail_on_engine_P) look at the blurred, normalised map through a bar of 1e-3 of its maximum, under which a cut that is
off by a few elements, or by the whole low 16 bits of the threshold, disappears.  Equality may be demanded because every precondition is a property
of the inputs that tests/test_tail_inputs.py proves without a device (the cumulative sum passes the target at a distance of >= 1e-7 of the total, no
sample sum lies within 1e-9 of a float32 rounding boundary): no case here is skipped or relaxed at run time.

Shapes (C, N, HW): (1, 1, 5) and (3, 2, 77) take the scalar paths, (65, 3, 260) the float4 paths with two channels to a histogram block (C > 64),
(130, 2, 1028) the float4 paths with a second turn of the row loop (HW / 4 = 257 > 256) and up to three channels a block.  Families: values over 20
binades with 30 % zeros, values that agree in their top 15 / top 7 mantissa bits (the last pass / the last two passes decide), small-integer ties.
Percentiles 0, 20, 50, 99.999, 100 (at 100 the select's "total fell short of the target" fallback may fire) and the contrastive form.

Value-only mutations of saliency.hip, each built into a library of its own and run once on the MI355X against the 26 cases of this file and the
two older tests (`parity` = test_truncation_tail_equals_reference_formula_on_engine_P, `layer` = the stem / avg_shortcut / mfm cases of
test_truncated_contrastive_tail_on_engine_P; their figures are max|d|/max of the blurred map against a bar of 1e-3), with what caught each:
  (a) trunc_select_kernel writes thr after pass 2 (low byte zero)     24 fail here: test_tail_equals_the_truth, all 16 cases (thr bits), and every
                                                                      other test but the two wiring cases, whose two sides run the same kernels;
                                                                      parity FAILS (3.1e-3), layer passes all three
  (b) contrast_kernel keeps m > t                                     26 fail here: test_tail_equals_the_truth, all 16 (the elements equal to the
                                                                      cut go to 0); the wiring cases too (at 100 nothing survives m > max);
                                                                      parity FAILS (2.4e-3), layer FAILS all three (2.0e-3 .. 2.0e-2)
  (c) trunc_hist_kernel without its final flush                       24 fail here: test_tail_equals_the_truth, all 16; parity FAILS (7.6e-2),
                                                                      layer FAILS all three (3.9e-2 .. 3.3e-1)
  (d) trunc_hist_kernel compares the prefix shifted by `shift`        24 fail here: test_tail_equals_the_truth, all 16; parity FAILS (8.9e-2),
                                                                      layer FAILS all three (6.0e-2 .. 8.1e-2)
  (e) the float4 path of sample_sums_kernel drops v.w                 13 fail here: test_tail_equals_the_truth at the 8 cases with HW % 4 == 0
                                                                      (float32(sums)), and the other tests at those shapes; parity FAILS
                                                                      (1.5e-3), layer FAILS avg_shortcut (1.0e-2) and passes stem and mfm, whose
                                                                      HW is odd
So each of the five fails here at every shape that runs the mutated line, with the kernel and the value named.  The prediction that (a), (b) and (d)
would slip under the older tests' bar did not hold on the small maps those tests use, where a few elements at the cut are a visible share of the
map: only (a) passed any of them (the three layer cases, missing parity's bar by a factor of 3).
"""
import ctypes

import numpy as np
import pytest
import torch

import layer_nets as L
import tail_inputs as T
from xfr_amd import _lib
from xfr_amd.engine import Engine

pytestmark = pytest.mark.gpu

CASES = [(f, s) for f in T.FAMILIES for s in T.SHAPES]
IDS = ['%s-%dx%dx%d' % ((f,) + s) for f, s in CASES]
FORMS = T.PERCENTILES + (None,)
_ENGINES = {}


@pytest.fixture(scope='module', autouse=True)
def _engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _engine(name, device):
    """An engine of the catalogue net `name` (tests/layer_nets.py); for the synthetic inputs it only carries the handle."""
    if name not in _ENGINES:
        case = L.BY_NAME[name]
        e = Engine(case.program(), 8, device)
        e.load_weights(case.params())
        _ENGINES[name] = e
    return _ENGINES[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(eng, P, pct):
    sums, thr, out = eng.contrast_tail(P, pct)
    return sums.cpu().numpy(), None if thr is None else thr.cpu().numpy(), out.cpu().numpy()


def _check(tag, got, t, C):
    """sums, thr, contrast of one call against the truth t; every figure is printed before it is asserted."""
    sums, thr, out = got
    err = np.abs(sums - t.S64) / t.S64
    print('%s: sums rel err %.2e' % (tag, err.max()))
    assert np.array_equal(_bits(sums.astype(np.float32)), _bits(t.S64.astype(np.float32))), '%s: float32(sums) %s, want %s' % (tag, sums, t.S64)
    assert (err <= 1e-12).all(), '%s: sums %s, want %s' % (tag, sums, t.S64)
    if t.thr is None:
        assert thr is None
    else:
        print('%s: thr %s, want %s' % (tag, ['%08x' % b for b in _bits(thr)], ['%08x' % b for b in _bits(t.thr)]))
        assert np.array_equal(_bits(thr), _bits(t.thr)), '%s: thr %s (%s), want %s (%s)' % (tag, thr, ['%08x' % b for b in _bits(thr)], t.thr,
                                                                                         ['%08x' % b for b in _bits(t.thr)])
    assert out.shape == t.out.shape and out.dtype == np.float32
    wrong = _bits(out) != _bits(t.out)
    print('%s: contrast differs in %d of %d elements, max |d| %.3e' % (tag, int(wrong.sum()), wrong.size, np.abs(out.astype(np.float64) - t.out64).max()))
    assert not wrong.any(), '%s: %d of %d contrast elements differ from the float32 restatement, first at %s: %r, want %r' % (
        tag, int(wrong.sum()), wrong.size, tuple(np.argwhere(wrong)[0]), out[wrong][0], t.out[wrong][0])
    assert (np.abs(out.astype(np.float64) - t.out64) <= (C + 1) * 2.0 ** -24 * t.out64).all(), tag


@pytest.mark.parametrize('family,shape', CASES, ids=IDS)
def test_tail_equals_the_truth(gpu_device, family, shape):
    """Every percentile and the contrastive form: sums, thresholds of every sample and the contrast."""
    eng = _engine('stem', gpu_device)
    P = torch.as_tensor(T.case(family, shape).copy()).to(gpu_device)
    for pct in FORMS:
        _check('%s %s pct %s' % (family, shape, pct), _run(eng, P, pct), T.case_truth(family, shape, pct), shape[0])


@pytest.mark.parametrize('shape', T.SHAPES, ids=['%dx%dx%d' % s for s in T.SHAPES])
def test_two_calls_in_a_row_give_identical_bits(gpu_device, shape):
    """The select's scratch (prefix, running totals, histograms) is re-initialised by every call: a second call sees the first one's leftovers
    otherwise.  The sums are compared in float32: the order of their float64 atomic adds is the device's."""
    eng = _engine('stem', gpu_device)
    P = torch.as_tensor(T.case('cluster16', shape).copy()).to(gpu_device)
    for pct in (50.0, 100.0):
        a, b = _run(eng, P, pct), _run(eng, P, pct)
        assert np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(_bits(a[2]), _bits(b[2]))
        assert np.array_equal(a[0].astype(np.float32), b[0].astype(np.float32))
        _check('second call %s pct %g' % (shape, pct), b, T.case_truth('cluster16', shape, pct), shape[0])


def test_three_samples_directly_after_one(gpu_device):
    """No state leaks between calls of different N on one engine."""
    eng = _engine('stem', gpu_device)
    small, big = ('ties', (1, 1, 5)), ('wide', (65, 3, 260))
    Ps, Pb = (torch.as_tensor(T.case(*k).copy()).to(gpu_device) for k in (small, big))
    for pct in (20.0, 99.999):
        one = _run(eng, Ps, pct)
        three = _run(eng, Pb, pct)
        _check('N = 1, pct %g' % pct, one, T.case_truth(*small, pct), 1)
        _check('N = 3 after N = 1, pct %g' % pct, three, T.case_truth(*big, pct), 65)


@pytest.mark.parametrize('family,shape', [('wide', (3, 2, 77)), ('ties', (65, 3, 260))])
def test_contrastive_form_leaves_thr_untouched(gpu_device, family, shape):
    """percentile < 0: no threshold launches; a thr_dev handed in all the same keeps its sentinel, the output is the restatement without a mask."""
    eng = _engine('stem', gpu_device)
    C, N, HW = shape
    P = torch.as_tensor(T.case(family, shape).copy()).to(gpu_device)
    sums = torch.full((2 * N,), -7.0, device=gpu_device, dtype=torch.float64)
    thr = torch.full((N,), -7.0, device=gpu_device)
    out = torch.full((N, HW), -7.0, device=gpu_device)
    with torch.cuda.device(gpu_device):
        _lib.check(eng.lib.xfr_debug_contrast_tail(eng._h, P.data_ptr(), C, N, HW, -1.0, sums.data_ptr(), thr.data_ptr(), out.data_ptr(),
                                                   ctypes.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)))
    torch.cuda.synchronize()
    assert (thr.cpu().numpy() == -7.0).all()
    _check('%s %s contrastive' % (family, shape), (sums.cpu().numpy(), None, out.cpu().numpy()), T.case_truth(family, shape, None), C)
    # without sums_dev and thr_dev the call keeps them in its own scratch: the same contrast
    out2 = torch.full((N, HW), -7.0, device=gpu_device)
    with torch.cuda.device(gpu_device):
        _lib.check(eng.lib.xfr_debug_contrast_tail(eng._h, P.data_ptr(), C, N, HW, 20.0, None, None, out2.data_ptr(),
                                                   ctypes.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)))
    assert np.array_equal(_bits(out2.cpu().numpy()), _bits(T.case_truth(family, shape, 20.0).out))


@pytest.mark.parametrize('name', ['stem', 'mfm'])
def test_engine_hands_the_tail_the_rows_the_hook_was_verified_with(gpu_device, name):
    """The real path: contrastive(raw=True) on three images equals the hook run on the engine's own P[-2] (xfr_ebp's MWP, permuted back to
    [C][2N][HW]) bit for bit -- both sides run the same kernels, so no margin is needed; a tail launched with other rows, counts or strides than
    the hook's would differ."""
    case = L.BY_NAME[name]
    eng = _engine(name, gpu_device)
    eng.set_mode('affineonly_with_prior')
    st = case.program().marks['classify']
    d = int(np.prod(eng.tensor_shape(st)))
    n = 3
    x = case.inputs(n, seed=3).to(gpu_device)
    seeds = torch.rand((2, n, d), generator=torch.Generator().manual_seed(31 * case.seed + 5)).to(gpu_device)
    mwp, _ = eng.ebp(x, st, seeds, want_mwp=True, want_pooled=False)
    c1, h1, w1 = eng.tensor_shape(1)
    P = mwp.permute(2, 0, 1, 3, 4).reshape(c1, 2 * n, h1 * w1).contiguous()
    assert float(P.sum()) > 0
    for pct in (20.0, 100.0, None):
        want = eng.contrastive(x, st, seeds, pct, raw=True).reshape(n, h1 * w1).cpu().numpy()
        got = eng.contrast_tail(P, pct)[2].cpu().numpy()
        assert np.isfinite(want).all() and want.max() > 0
        assert np.array_equal(_bits(got), _bits(want)), '%s pct %s: %d elements differ' % (name, pct, int((_bits(got) != _bits(want)).sum()))


def test_argument_errors(gpu_device):
    """Every refusal of include/xfr_amd.h, with the value in the text and nothing launched: the sentinel-filled outputs and P are as they were."""
    eng = _engine('stem', gpu_device)
    C, N, HW = 3, 2, 8
    host = np.arange(C * 2 * N * HW + 4, dtype=np.float32) + 1
    buf = torch.as_tensor(host).to(gpu_device)
    sums = torch.full((2 * N,), -7.0, device=gpu_device, dtype=torch.float64)
    thr = torch.full((N,), -7.0, device=gpu_device)
    out = torch.full((N, HW), -7.0, device=gpu_device)
    p = buf.data_ptr()
    assert p % 16 == 0
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)

    def refused(pattern, e=eng._h, p_dev=p, c=C, n=N, hw=HW, pct=20.0, s=sums.data_ptr(), t=thr.data_ptr(), o=out.data_ptr()):
        with torch.cuda.device(gpu_device):
            status = eng.lib.xfr_debug_contrast_tail(e, p_dev, c, n, hw, pct, s, t, o, stream)
        assert status == _lib.XFR_INVALID_ARG, (pattern, status)
        with pytest.raises(ValueError, match=pattern):
            _lib.check(status)

    refused('debug_contrast_tail: null argument', e=None)
    refused('debug_contrast_tail: null argument', p_dev=None)
    refused('debug_contrast_tail: null argument', o=None)
    refused(r'c 0, n 2, hw 8', c=0)
    refused(r'c 3, n 0, hw 8', n=0)
    refused(r'c 3, n 2, hw -1', hw=-1)
    refused(r'n 40000', n=40000)
    refused(r'percentile 100\.5', pct=100.5)
    refused(r'percentile -?nan', pct=float('nan'))
    refused(r'p_dev 0x[0-9a-f]+ is not 16-byte aligned', p_dev=p + 4)
    refused(r'sums_dev 0x[0-9a-f]+ \(32 bytes\) overlaps p_dev', s=p + 16)
    refused(r'thr_dev 0x[0-9a-f]+ \(8 bytes\) overlaps p_dev', t=p + 4 * (C * 2 * N * HW) - 4)
    refused(r'contrast_dev 0x[0-9a-f]+ \(64 bytes\) overlaps p_dev', o=p)
    torch.cuda.synchronize()
    assert (sums.cpu().numpy() == -7.0).all() and (thr.cpu().numpy() == -7.0).all() and (out.cpu().numpy() == -7.0).all()
    assert np.array_equal(buf.cpu().numpy(), host)
    # and the same arguments un-refused run: an output that ends where P begins, or begins where it ends, does not overlap
    with torch.cuda.device(gpu_device):
        _lib.check(eng.lib.xfr_debug_contrast_tail(eng._h, p, C, N, HW, 20.0, sums.data_ptr(), p + 4 * (C * 2 * N * HW), out.data_ptr(), stream))
    P = host[:C * 2 * N * HW].reshape(C, 2 * N, HW)
    t = T.truth(P, N, 20.0)
    assert t.gap.min() >= T.GAP_MIN and t.sum_margin.min() >= T.SUM_MARGIN_MIN      # a property of arange, decided on the CPU
    _check('arange', (sums.cpu().numpy(), buf[C * 2 * N * HW:C * 2 * N * HW + N].cpu().numpy(), out.cpu().numpy()), t, C)
