"""The truth of the uint8 saliency tail (tests/u8_tail_inputs.py) held to the installed NumPy and Pillow, to the byte, without a device: it documents
that the restatement IS the reference's chain -- Whitebox._mwp_to_saliency's host branch -- on every case the GPU test runs, and guards the two
places where a plausible shortcut is wrong (the float64 form of the uint8 stretch; the engine's eps, a float widened to double)."""
import numpy as np
import PIL.Image
import PIL.ImageFilter
import pytest

import u8_tail_inputs as U

ALL = [(f, s) for s in U.SHAPES for f in U.F32_FAMILIES + U.U8_FAMILIES]
IDS = ['%s-%dx%d' % ((f,) + s) for f, s in ALL]


class _Host(object):
    """Whitebox._mwp_to_saliency needs nothing of a Whitebox but eps and the version switch on its host branch."""
    convert_saliency_uint8 = True

    def __init__(self, eps):
        self.eps = eps


def _host_chain(img, eps):
    from xfr_amd.models.whitebox import Whitebox
    return Whitebox._mwp_to_saliency(_Host(eps), img)


@pytest.mark.parametrize('family,shape', ALL, ids=IDS)
def test_truth_is_the_host_branch(family, shape):
    img = U.case(family, shape)
    for eps in U.EPS:
        want = _host_chain(np.array(img), eps)
        got = U.case_truth(family, shape, eps)
        assert got.dtype == want.dtype == np.uint8 and got.shape == want.shape == shape
        assert np.array_equal(got, want), '%s %s eps %g: %d bytes differ' % (family, shape, eps, int((got != want).sum()))


@pytest.mark.parametrize('family,shape', ALL, ids=IDS)
def test_blur_truth_is_pillows(family, shape):
    img = U.case(family, shape)
    a = U.stretch_u8(img, 1e-16) if img.dtype == np.uint8 else U.stretch_f32(img, 1e-16)
    want = np.array(PIL.Image.fromarray(a).filter(PIL.ImageFilter.GaussianBlur(radius=2)))
    assert np.array_equal(U.pil_gaussian_blur_2(a), want)


def test_stage_a_forms_are_numpys():
    """The two forms of the first stretch against the reference's expression itself under the installed NumPy."""
    expr = lambda img, eps: np.uint8(255 * ((img - np.min(img)) / (eps + (np.max(img) - np.min(img)))))          # noqa: E731
    for family, shape in ALL:
        img = np.array(U.case(family, shape))
        for eps in U.EPS:
            got = U.stretch_u8(img, eps) if img.dtype == np.uint8 else U.stretch_f32(img, eps)
            assert np.array_equal(got, expr(img, eps)), (family, shape, eps)


def test_uint8_form_is_float64_not_an_integer_floor():
    """At eps = 1e-12 the identity 0..255 comes back one level lower, maximum 254; at 1e-16 it is floor(255 v / d) for every v <= d."""
    low = U.stretch_u8(U.IDENTITY, 1e-12)
    assert int(low.max()) == 254
    assert np.array_equal(low.ravel()[1:], np.arange(255, dtype=np.uint8))
    assert np.array_equal(U.stretch_u8(U.IDENTITY, 1e-16), U.IDENTITY)
    for d in range(1, 256):
        v = np.arange(d + 1, dtype=np.uint8)
        assert np.array_equal(U.stretch_u8(v, 1e-16), (255 * v.astype(np.int64)) // d), d


def test_float_eps_widened_to_double_rounds_as_the_double_literal():
    """The engine holds eps as a float (xfr_engine_set_mode) and the uint8 form widens it: for the two values of eps in use, eps + d is the same
    double for every d = 1..255 (and d = 0 divides 0 by either), so the levels are those of the host's double eps."""
    for eps in U.EPS:
        wide = np.float64(np.float32(eps))
        assert wide != np.float64(eps)
        for d in range(1, 256):
            assert np.float64(eps) + np.float64(d) == wide + np.float64(d), (eps, d)


def test_families_are_what_they_claim():
    for shape in U.SHAPES:
        assert U.case('constant', shape).max() == U.case('constant', shape).min()
        b = U.case('below_eps', shape)
        assert float(b.max()) - float(b.min()) < 1e-19 and not U.case_truth('below_eps', shape, 1e-16).any()
        assert U.case('negative', shape).min() < 0 or shape == (1, 1)
        assert not U.case_truth('constant', shape, 1e-12).any() and not U.case_truth('constant_bytes', shape, 1e-12).any()
        if shape[0] * shape[1] > 1:
            d1 = U.case('d1', shape)
            assert int(d1.max()) - int(d1.min()) == 1
    s = U.case('steps', (113, 97))
    q = np.float32(255.0) * ((s - s.min()) / (np.float32(1e-16) + (s.max() - s.min())))
    assert q.dtype == np.float32
    near = np.abs(q - np.round(q)) < 1e-3
    assert near.mean() > 0.9 and (q == np.round(q)).any() and (q < np.round(q)).any() and (q > np.round(q)).any()
    assert len(np.unique(U.case('ramp', (113, 97)))) == 256
