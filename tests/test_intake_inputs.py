"""Image intake on the host: xfr_amd.intake.host_bytes -- the numpy statement the kernels of csrc/intake.hip restate -- against the parent's chain
(image_loader + Whitebox.convert_from_numpy: saliency_io.resize_linear and the truncation to bytes), byte for byte; its pre-filter against scipy to
the float bit; intake_items against image_loader on files and DataFrame rows; the Light-CNN stage against PIL.  No device."""
import types

import numpy as np
import PIL.Image
import pytest
import scipy.ndimage as ndi

import intake_inputs as I
from xfr_amd import image_loader as IL
from xfr_amd import intake
from xfr_amd.models import whitebox as WB
from xfr_amd.models.blackbox import apply_pil_tables, pil_bilinear_tables
from xfr_amd.models.lightcnn import lightcnn_preprocess, prepare_lightCNN_image


@pytest.mark.parametrize('head', I.HEADS)
@pytest.mark.parametrize('channels', I.CHANNELS)
@pytest.mark.parametrize('case', I.CASES, ids=I.case_id)
def test_host_bytes_equal_the_parents_chain(case, channels, head):
    for u, want in I.truth(case, channels, head):
        got = intake.host_bytes(u, case[1], head)
        assert got.dtype == np.uint8 and got.shape == tuple(case[1]) + (3,)
        assert np.array_equal(got, want), '%d of %d bytes differ' % (int((got != want).sum()), want.size)
    if channels == 1:                                                  # a grey crop may come without its channel axis
        u = I.truth(case, 1, head)[0][0]
        assert np.array_equal(intake.host_bytes(u[:, :, 0], case[1], head), I.truth(case, 1, head)[0][1])


def test_heads_differ_where_they_should():
    """The two heads are not interchangeable: they give different bytes at 96 -> 224, and the float32 same-size path is not the identity."""
    u = I.random_image(96, 96, 3, seed=7)
    a, b = intake.host_bytes(u, (224, 224), intake.HEAD_F64), intake.host_bytes(u, (224, 224), intake.HEAD_F32)
    assert 0 < int((a != b).sum()) < a.size // 10
    v = I.all_values(224, 224, 3)
    same = intake.host_bytes(v, (224, 224), intake.HEAD_F32)
    assert np.array_equal(same, ((v.astype(np.float32) / 255) * 255).astype(np.uint8))


@pytest.mark.parametrize('case', [c for c in I.CASES if c[0][0] > c[1][0] or c[0][1] > c[1][1]], ids=I.case_id)
def test_prefilter_equals_scipy_to_the_bit(case):
    (h, w), out = case
    for u in I.images_of(case, 3):
        a = intake.head(u, intake.HEAD_F64)
        factors = np.divide((h, w), out)
        got = intake.prefilter(a, out)
        for c in range(3):
            want = ndi.gaussian_filter(a[..., c], np.maximum(0, (factors - 1) / 2), mode='mirror')
            assert np.array_equal(got[..., c], want), np.abs(got[..., c] - want).max()


def test_refusals_name_the_reason():
    assert intake.refusal((5, 5, 2), (4, 4)) == '2 channels'
    assert 'radius' in intake.refusal((4000, 8, 3), (8, 8))
    assert intake.refusal((40, 5, 3), (4, 4)) is None
    assert intake.prefilter_of(40, 4) == (4.5, 18) and intake.prefilter_of(8, 1) == (3.5, 14) and intake.prefilter_of(9, 4)[1] == 3
    with pytest.raises(intake.IntakeRefused):
        intake.host_bytes(np.zeros((5, 5, 2), np.uint8), (4, 4), intake.HEAD_F64)
    with pytest.raises(ValueError):
        intake.host_bytes(np.zeros((5, 5, 3), np.float32), (4, 4), intake.HEAD_F64)
    # every size the zoom would round away from is refused, and those it keeps are not: the rule is scipy's own
    for n, m in ((7, 16), (300, 224), (421, 224), (3, 2), (5, 224)):
        z = ndi.zoom(np.zeros(n), 1.0 / (np.float64(n) / m), order=1, mode='mirror', grid_mode=True)
        assert intake.zoom_keeps_size(n, m) == (z.shape[0] == m)


def _parent_bytes_of(images):
    """The bytes convert_from_numpy hands to the network's preprocess for what image_loader yields: the parent's chain itself, with a network
    whose preprocess returns the PIL image it is given."""
    seen = []
    fake = types.SimpleNamespace(net=types.SimpleNamespace(preprocess=lambda im: seen.append(np.asarray(im).copy()) or [None]))
    for im in IL.image_loader(images):
        WB.Whitebox.convert_from_numpy(fake, im)
    return seen


def _intake_bytes_of(images):
    items = list(IL.intake_items(images))
    assert all(it is not None for it in items)
    return [intake.host_bytes(u, (IL.NET_SIDE, IL.NET_SIDE), head) for u, head in items]


def _write_files(tmp_path):
    rs = np.random.RandomState(11)
    grey = rs.randint(0, 256, size=(50, 41)).astype(np.uint8)
    rgb = rs.randint(0, 256, size=(224, 260, 3)).astype(np.uint8)
    rgba = rs.randint(0, 256, size=(61, 47, 4)).astype(np.uint8)
    small = I.ramp(230, 231, 3)
    pal = PIL.Image.fromarray(rs.randint(0, 256, size=(40, 52, 3)).astype(np.uint8)).convert('P')
    names = {}
    for name, im in (('grey', PIL.Image.fromarray(grey)), ('rgb', PIL.Image.fromarray(rgb)), ('rgba', PIL.Image.fromarray(rgba)),
                     ('ramp', PIL.Image.fromarray(small)), ('pal', pal)):
        names[name] = str(tmp_path / (name + '.png'))
        im.save(names[name])
    return names


def test_files_give_the_parents_bytes(tmp_path):
    names = _write_files(tmp_path)
    fns = [names[k] for k in ('grey', 'rgb', 'rgba', 'ramp', 'pal')]
    want, got = _parent_bytes_of(fns), _intake_bytes_of(fns)
    assert len(want) == len(got) == 5
    for fn, w, g in zip(fns, want, got):
        assert w.shape == (224, 224, 3) and np.array_equal(w, g), '%s: %d bytes differ' % (fn, int((w != g).sum()))
    heads = [it[1] for it in IL.intake_items(fns)]
    assert heads == [intake.HEAD_F64] * 5
    assert [it[0].shape for it in IL.intake_items(fns)] == [(41, 41), (224, 224, 3), (47, 47, 4), (230, 230, 3), (40, 40, 3)]


def test_dataframe_rows_give_the_parents_bytes(tmp_path):
    pd = pytest.importorskip('pandas')
    names = _write_files(tmp_path)
    rs = np.random.RandomState(12)
    big = str(tmp_path / 'big.png')
    PIL.Image.fromarray(rs.randint(0, 256, size=(300, 400, 3)).astype(np.uint8)).save(big)
    boxed = pd.DataFrame([dict(Filename=big, SubjectID='a', XMin=30, YMin=20, Width=120, Height=150),
                          dict(Filename=big, SubjectID='b', XMin=200, YMin=100, Width=260, Height=250),      # pushed back inside the image
                          dict(Filename=names['rgba'], SubjectID='c', XMin=5, YMin=6, Width=30, Height=20)])
    bare = pd.DataFrame([dict(Filename=names['grey'], SubjectID='d'), dict(Filename=names['rgb'], SubjectID='e')])      # no box: the whole image
    for frame in (boxed, bare):
        want, got = _parent_bytes_of(frame), _intake_bytes_of(frame)
        assert len(want) == len(got) == len(frame)
        for w, g in zip(want, got):
            assert np.array_equal(w, g), '%d bytes differ' % int((w != g).sum())


def test_arrays_uint8_take_the_float32_head_and_floats_stay_on_the_host():
    u = [I.random_image(224, 224, 3, seed=3), I.random_image(96, 131, 3, seed=4)]
    items = list(IL.intake_items(u))
    assert [it[1] for it in items] == [intake.HEAD_F32] * 2 and items[0][0] is u[0]
    assert all(np.array_equal(w, g) for w, g in zip(_parent_bytes_of(u), _intake_bytes_of(u)))
    floats = [u[0].astype(float) / 255, u[1].astype(np.float32)]
    assert list(IL.intake_items(floats)) == [None, None]
    assert list(IL.intake_items([u[0], floats[0]]))[1] is None


def _pil_resize_crop(b, resize_short, crop):
    """lightcnn_preprocess's Resize + CenterCrop on uint8 RGB bytes, with PIL itself."""
    im = PIL.Image.fromarray(b)
    w, h = im.size
    nw, nh = (resize_short, int(resize_short * h / w)) if w <= h else (int(resize_short * w / h), resize_short)
    im = im.resize((nw, nh), PIL.Image.BILINEAR)
    left, top = int(round((nw - crop) / 2.0)), int(round((nh - crop) / 2.0))
    return np.asarray(im.crop((left, top, left + crop, top + crop)))


@pytest.mark.parametrize('hw, resize_short, crop', [((224, 224), 144, 128), ((10, 9), 6, 4)])
def test_lightcnn_stage_equals_pil(hw, resize_short, crop):
    for b in (I.random_image(hw[0], hw[1], 3, seed=21), I.ramp(hw[0], hw[1], 3)):
        tables = pil_bilinear_tables(hw, resize_short, (crop, crop))
        got = intake.host_chain_bytes([(b, intake.HEAD_F32)], hw, tables)[0]
        assert np.array_equal(got, _pil_resize_crop(b, resize_short, crop))
        if resize_short == 144:
            import torch
            assert torch.equal(prepare_lightCNN_image(PIL.Image.fromarray(got)), lightcnn_preprocess()(PIL.Image.fromarray(b)))


def test_pack_lays_out_every_crop():
    big = I.random_image(30, 40, 3, seed=5)
    crops = [(big[3:20, 5:30], intake.HEAD_F64), (I.random_image(4, 5, 1, seed=6)[:, :, 0], intake.HEAD_F32), (I.random_image(2, 3, 4, seed=7), intake.HEAD_F64)]
    src, table = intake.pack(crops)
    assert src.dtype == np.uint8 and src.size == 17 * 25 * 3 + 4 * 5 + 2 * 3 * 4 and len(table) == 3
    for (u, head), it in zip(crops, table):
        c = u.shape[2] if u.ndim == 3 else 1
        assert (it.h, it.w, it.channels, it.head, it.row_stride) == (u.shape[0], u.shape[1], c, head, u.shape[1] * c)
        assert np.array_equal(src[it.offset:it.offset + u.size].reshape(u.shape), u)
    sig, rad, wts = intake.stated_kernels([(I.random_image(40, 5, 3, seed=8), 0), (I.random_image(9, 11, 3, seed=9), 0)], (4, 4))
    assert wts.shape == (len(sig), intake.MAX_RADIUS + 1) and sorted(rad) == [1, 3, 4, 18]      # 5 -> 4, 9 -> 4, 11 -> 4, 40 -> 4
    for s_, r_, w_ in zip(sig, rad, wts):
        assert np.array_equal(w_[:r_ + 1], intake.gaussian_weights(s_, r_)[:r_ + 1]) and not w_[r_ + 1:].any()
