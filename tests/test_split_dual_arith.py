"""The mask rule of the bf16x6 kernel's two-accumulator (DUAL) instantiation (conv_gemm_split.hip relu_pieces), restated in numpy.

The kernel holds a weight as three bf16 pieces, W = p0 + p1 + p2, each the round-to-nearest bf16 of what the pieces before it left (split_pair).
The relu(W) tile is multiplied from the W fragments in registers: with m = all ones where p0 < 0 (the sign bit of p0 spread over its 16 bits),
r_i = p_i & ~m.  p0 is the rounded weight and carries its sign, so the r_i are exactly the pieces of relu(W).  Clamping every piece by its OWN sign,
max(p_i, 0), is another function: p1 and p2 are signed remainders, and a positive weight has a negative p1 about half the time.  The sample below
holds thousands of weights of every sign combination of (p0, p1), exact zeros of both signs and the smallest normal numbers; the first rule is
exact on all of it, the second is shown to fail on it.
"""
import numpy as np


def bf16_rn(x):
    """Round-to-nearest-even bf16 of float32 values, as float32 (v_cvt_pk_bf16_f32; no NaN / Inf in the sample)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return r.astype(np.uint32).view(np.float32)


def split_pair(w):
    """The three pieces of split_pair (conv_gemm_split.hip): both remainders are exact in float32."""
    p0 = bf16_rn(w)
    r = (w - p0).astype(np.float32)
    p1 = bf16_rn(r)
    s = (r - p1).astype(np.float32)
    p2 = bf16_rn(s)
    return p0, p1, p2


def bits16(p):
    """The bf16 bit pattern of a float32 that holds a bf16 value."""
    u = np.ascontiguousarray(p, dtype=np.float32).view(np.uint32)
    assert not (u & 0xffff).any()
    return (u >> 16).astype(np.uint16)


def from_bits16(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def mask_rule(p0, p1, p2):
    """r_i = p_i & ~m with m = p0 >> 15 (arithmetic, 16 bits): the kernel's rule, on the bit patterns."""
    m = (bits16(p0).view(np.int16) >> 15).view(np.uint16)
    return tuple(from_bits16(bits16(p) & ~m) for p in (p0, p1, p2))


def sum3(a, b, c):
    """The sum of three pieces in float64 (exact: they span fewer than 53 bits), and its float32 rounding."""
    s = a.astype(np.float64) + b.astype(np.float64) + c.astype(np.float64)
    return s, s.astype(np.float32)


def sample():
    rng = np.random.RandomState(20260)
    parts = [
        rng.standard_normal(200000).astype(np.float32),                                               # weights as a layer holds them
        (rng.standard_normal(50000) * np.exp(rng.uniform(-60, 20, 50000))).astype(np.float32),         # every scale
        np.zeros(64, np.float32), -np.zeros(64, np.float32),                                           # exact zeros of both signs
    ]
    tiny = np.float32(2.0) ** -126                                                                     # the smallest normal number and its neighbours
    # (seven mantissa bits: down there bf16 itself is denormal with a last bit of 2^-133, and three pieces cannot hold more than float32's own
    # bits above that)
    mant = (1.0 + rng.randint(0, 128, 2000) / 128.0).astype(np.float32)
    parts += [np.array([tiny, -tiny], np.float32), (tiny * mant).astype(np.float32), (-tiny * mant).astype(np.float32)]
    w = np.concatenate(parts).astype(np.float32)
    assert np.isfinite(w).all()
    return w


def test_pieces_sum_to_the_weight():
    w = sample()
    p0, p1, p2 = split_pair(w)
    s64, s32 = sum3(p0, p1, p2)
    assert np.array_equal(s64, w.astype(np.float64)) and np.array_equal(s32, w)


def test_sample_holds_every_sign_combination():
    """The sample the other tests run on: >= 1000 weights for each sign of p0 with each sign of p1, zeros, the smallest normals."""
    w = sample()
    p0, p1, _ = split_pair(w)
    for s0 in (1, -1):
        for s1 in (1, -1):
            n = int(((np.sign(p0) == s0) & (np.sign(p1) == s1)).sum())
            assert n >= 1000, (s0, s1, n)
    assert int((w == 0).sum()) >= 128 and int(np.signbit(w[w == 0]).sum()) >= 64
    assert int((np.abs(w) == np.float32(2.0) ** -126).sum()) >= 2
    assert int(((np.abs(w) >= np.float32(2.0) ** -126) & (np.abs(w) < np.float32(2.0) ** -125)).sum()) >= 4000


def test_mask_rule_gives_the_pieces_of_relu_w():
    w = sample()
    relu = np.where(w > 0, w, np.float32(0)).astype(np.float32)
    r = mask_rule(*split_pair(w))
    s64, s32 = sum3(*r)
    assert np.array_equal(s64, relu.astype(np.float64)), 'r0 + r1 + r2 != relu(W)'
    assert np.array_equal(s32, relu)
    # ... piece by piece what the split of relu(W) itself gives (as values: the split of -0.0 and of 0.0 differ in sign bits only)
    for got, want in zip(r, split_pair(relu)):
        assert np.array_equal(got, want)


def test_per_piece_clamp_is_another_function():
    """max(p_i, 0) piece by piece: wrong on EVERY weight whose p1 has the other sign than p0 -- the test can tell the two rules apart."""
    w = sample()
    relu = np.where(w > 0, w, np.float32(0)).astype(np.float32)
    p0, p1, p2 = split_pair(w)
    c = tuple(np.maximum(p, np.float32(0)) for p in (p0, p1, p2))
    s64, _ = sum3(*c)
    wrong = s64 != relu.astype(np.float64)
    pos_neg = (p0 > 0) & (p1 < 0)
    neg_pos = (p0 < 0) & (p1 > 0)
    assert int(pos_neg.sum()) >= 1000 and int(neg_pos.sum()) >= 1000
    assert wrong[pos_neg].all(), 'a positive weight with a negative p1 survived the per-piece clamp'
    assert wrong[neg_pos].all(), 'a negative weight with a positive p1 survived the per-piece clamp'
    # ... and the mask rule is right on exactly those
    m64, _ = sum3(*mask_rule(p0, p1, p2))
    assert np.array_equal(m64[wrong], relu.astype(np.float64)[wrong])
