"""What tests/test_tail_inputs.py and tests/test_gpu_contrast_tail.py share: seeded inputs P[C][2N][HW] for the tail of the truncated contrastive
EBP (xfr_debug_contrast_tail: sample sums, radix-select threshold, contrast) and its exact truth in NumPy.  A plain module, no test in it, no device.

The tail is the one place of the hot path whose right answer is exactly computable: the quotient m = P / S is one correctly rounded float32 division,
the threshold is an element of m, and the contrast is a handful of float32 operations none of which can be contracted.  So the truth here is held to
the bit, and the only freedom the device has -- the order of its float64 additions -- is kept away from every decision by two margins that are
properties of the inputs alone (`gap`, `sum_margin`), asserted on the CPU by test_tail_inputs.py."""
import functools
import math

import numpy as np

FAMILIES = ('wide', 'cluster', 'cluster16', 'ties')
# (C, N, HW), the smallest that reach each code path: the scalar path; the scalar path with HW < 256; float4 with C > 64 (a block of the histogram
# takes two channels); float4 with HW / 4 = 257 > 256 (the row loop runs twice) and two or three channels a block
SHAPES = ((1, 1, 5), (3, 2, 77), (65, 3, 260), (130, 2, 1028))
PERCENTILES = (0.0, 20.0, 50.0, 99.999, 100.0)
GAP_MIN = 1e-7            # thirty times |20/100 in float32 - in float64|, six orders above float64 summation noise
SUM_MARGIN_MIN = 1e-9     # far above any order-dependent float64 rounding of the device's atomic adds
# seed of a case: C + HW unless a draw of that seed misses a margin or leaves a sample empty (test_tail_inputs.py decides); then the first
# C + HW + 1000 k, k = 1, 2, ..., that holds them all
SEED_OVERRIDES = {('wide', (3, 2, 77)): 1080, ('cluster', (1, 1, 5)): 1006, ('ties', (130, 2, 1028)): 2158}


def _draw(family, rng, shape):
    """Non-negative float64 values of one sample, every one a float32."""
    if family == 'wide':          # zero-heavy, spread over 20 binades
        v = rng.rand(*shape) ** 8 * 2.0 ** rng.randint(-20, 1, shape)
        v[rng.rand(*shape) < 0.3] = 0.0
        v = v.astype(np.float32).astype(np.float64)
        v[v < 2.0 ** -60] = 0.0          # with S < 2^20 no quotient other than 0 falls below 2^-100: no subnormals
        return v
    if family == 'cluster':       # after the division the values agree in their top 15 mantissa bits: passes 0-2 see one bin, the last pass decides
        return 1.0 + rng.randint(0, 256, shape) * 2.0 ** -23
    if family == 'cluster16':     # ... in their top 7 bits: the last two passes decide
        return 1.0 + rng.randint(0, 65536, shape) * 2.0 ** -23
    if family == 'ties':          # the cut value has multiplicity in the hundreds
        return rng.randint(0, 6, shape).astype(np.float64)
    raise KeyError(family)


def seed_of(family, shape):
    C, _, HW = shape
    return SEED_OVERRIDES.get((family, shape), C + HW)


def make_P(family, shape, seed=None):
    """float32 P[C][2N][HW].  Sample j of the mate half draws from family number (f + j) % 4 with f the case's own, so that per-sample indexing
    shows; row N + j from family (f + j + 1) % 4 scaled by 3, so that the non-mate half has other totals and reading the wrong half shows."""
    C, N, HW = shape
    rng = np.random.RandomState(seed_of(family, shape) if seed is None else seed)
    f = FAMILIES.index(family)
    P = np.empty((C, 2 * N, HW), dtype=np.float32)
    for j in range(N):
        P[:, j, :] = _draw(FAMILIES[(f + j) % 4], rng, (C, HW))
        P[:, N + j, :] = 3.0 * _draw(FAMILIES[(f + j + 1) % 4], rng, (C, HW))
    return P


@functools.lru_cache(maxsize=None)
def case(family, shape):
    """The input of a (family, shape) case, read-only: computed once, shared by every test."""
    P = make_P(family, shape)
    P.setflags(write=False)
    return P


class Truth(object):
    """S64 [2N] float64, the exact sums; m [C][2N][HW] float32, the quotients; thr [N] float32 (None in the contrastive form); out [N][HW] float32,
    the contrast to the bit; out64 [N][HW], the same sum in float64; gap [N], sum_margin [2N]."""


def _sum_margin(S64):
    """Distance of S64 from the nearest point where float32(S64) changes, in units of S64."""
    s = np.float32(S64)
    up = (np.float64(s) + np.float64(np.nextafter(s, np.float32(np.inf)))) / 2
    dn = (np.float64(s) + np.float64(np.nextafter(s, np.float32(-np.inf)))) / 2
    return min(abs(S64 - up), abs(S64 - dn)) / S64


def truth(P, N, percentile):
    """The tail of whitebox.py:524-526 (percentile None) / :547-557 on P[C][2N][HW], as the library states it: m = float32(P) / float32(S), the
    threshold v* = sort(m_n)[i*] with i* the first index at which the float64 cumulative sum of the ascending values reaches
    (float64(float32(pct)) / 100) * total, keep = (m >= v*) -- every tie of the cut value is kept --, out = sum over c ascending of
    max(float32(m - q), 0) in float32."""
    P = np.asarray(P)
    assert P.dtype == np.float32 and P.ndim == 3 and P.shape[1] == 2 * N
    C, SB, HW = P.shape
    t = Truth()
    t.S64 = np.array([math.fsum(P[:, sb, :].astype(np.float64).ravel()) for sb in range(SB)])
    t.sum_margin = np.array([_sum_margin(S) for S in t.S64])
    s = t.S64.astype(np.float32)
    t.m = P / s[None, :, None]
    assert t.m.dtype == np.float32
    t.thr = None if percentile is None else np.empty(N, dtype=np.float32)
    t.gap = np.full(N, np.inf)
    t.out = np.empty((N, HW), dtype=np.float32)
    t.out64 = np.empty((N, HW), dtype=np.float64)
    for n in range(N):
        m, q = t.m[:, n, :], t.m[:, N + n, :]
        d = m - q
        if percentile is not None:
            v = np.sort(m.ravel())
            cs = np.cumsum(v.astype(np.float64))
            target = (np.float64(np.float32(percentile)) / 100) * cs[-1]
            t.thr[n] = v[int(np.argmax(cs >= target))]
            t.gap[n] = np.abs(cs - target).min() / cs[-1]
            d = np.where(m >= t.thr[n], d, np.float32(0))
        r = np.maximum(d, np.float32(0))
        acc = np.zeros(HW, dtype=np.float32)
        for c in range(C):
            acc = acc + r[c]
        t.out[n] = acc
        t.out64[n] = r.astype(np.float64).sum(axis=0)
    return t


@functools.lru_cache(maxsize=None)
def case_truth(family, shape, percentile):
    return truth(case(family, shape), shape[1], percentile)


def reference_mask(m, percentile):
    """whitebox.py:550-554 on the quotients of one sample, restated in float64: the ascending sort, the cumulative sum, the mask scattered back."""
    flat = m.ravel()
    idx = np.argsort(flat, kind='stable')
    cs = np.cumsum(flat[idx].astype(np.float64))
    mask = np.zeros(flat.shape, dtype=bool)
    mask[idx] = cs >= (percentile / 100.0) * cs[-1]
    return mask.reshape(m.shape)
