"""GPU tests of image intake: the kernels of intake.hip through the C ABI (xfr_intake_u8, xfr_intake_u8_host), Engine.intake_u8, Whitebox.intake
and the `intake` option of Whitebox.embeddings.

The truth is xfr_amd.intake.host_bytes, which tests/test_intake_inputs.py holds to the parent's chain byte for byte.  The bar is equality of every
byte: the device runs the same float64 operations in the same order, with the Gaussian weights the host states (Engine.intake_set_kernels)."""
import ctypes

import numpy as np
import pytest
import torch

import intake_inputs as I
from probe_scoring_utils import lcnn, mini32      # noqa: F401 (fixtures)
from xfr_amd import _lib
from xfr_amd import intake
from xfr_amd.models.blackbox import pil_bilinear_tables

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng(mini32):
    return mini32._engine(mini32.batch_size)


def _device(eng, crops, out_hw, tables=None, on_device=False):
    """crops [(uint8 array, head)] through one call, from host memory or from a device copy; every byte of the result goes into the comparison."""
    src, table = intake.pack(crops)
    eng.intake_set_kernels(*intake.stated_kernels(crops, out_hw))
    out = eng.intake_u8(torch.from_numpy(src).to(eng.device) if on_device else src, table, out_hw, tables=tables)
    assert out.dtype == torch.uint8 and out.is_cuda
    return out.cpu().numpy()


@pytest.mark.parametrize('channels', I.CHANNELS)
@pytest.mark.parametrize('case', I.CASES, ids=I.case_id)
def test_every_case_equals_host_bytes(eng, case, channels):
    crops = [(u, head) for head in I.HEADS for u in I.images_of(case, channels)]
    want = np.stack([intake.host_bytes(u, case[1], head) for u, head in crops])
    for on_device in (False, True):
        got = _device(eng, crops, case[1], on_device=on_device)
        assert got.shape == want.shape
        diff = int((got != want).sum())
        print('%s C=%d %s: %d of %d bytes differ' % (I.case_id(case), channels, 'device' if on_device else 'host', diff, want.size))
        assert diff == 0


def _ragged():
    shapes = [(96, 131, 3), (300, 280, 4), (224, 224, 3), (57, 40, 1), (421, 333, 3)]
    return [(I.random_image(h, w, c, seed=50 + k) if k % 2 else I.ramp(h, w, c), I.HEADS[k % 2]) for k, (h, w, c) in enumerate(shapes)]


def test_a_ragged_batch_equals_each_crop_alone_and_reversed(eng):
    crops = _ragged()
    out = (224, 224)
    batch = _device(eng, crops, out)
    want = np.stack([intake.host_bytes(u, out, head) for u, head in crops])
    assert np.array_equal(batch, want)
    for k, crop in enumerate(crops):
        assert np.array_equal(_device(eng, [crop], out)[0], batch[k])
    assert np.array_equal(_device(eng, crops[::-1], out)[::-1], batch)
    assert np.array_equal(_device(eng, crops, out, on_device=True), batch)      # the _host variant equals the device variant


def test_items_with_a_stride_and_an_offset_inside_a_larger_image(eng):
    big = I.random_image(260, 310, 3, seed=9)
    boxes = [(10, 170, 20, 180), (0, 260, 0, 310), (100, 101, 7, 8), (5, 250, 30, 130)]
    table = (intake.Item * len(boxes))()
    for k, (t, b, l, r) in enumerate(boxes):
        table[k] = intake.Item((t * 310 + l) * 3, b - t, r - l, 310 * 3, 3, I.HEADS[k % 2])
    crops = [(big[t:b, l:r], I.HEADS[k % 2]) for k, (t, b, l, r) in enumerate(boxes)]
    eng.intake_set_kernels(*intake.stated_kernels(crops, (224, 224)))
    want = np.stack([intake.host_bytes(u, (224, 224), head) for u, head in crops])
    for src in (big.reshape(-1), torch.from_numpy(big.reshape(-1)).to(eng.device)):
        assert np.array_equal(eng.intake_u8(src, table, (224, 224)).cpu().numpy(), want)


def test_the_table_stage_equals_the_host(eng):
    crops = _ragged()
    for hw, short, crop in (((224, 224), 144, 128), ((10, 9), 6, 4)):
        tables = pil_bilinear_tables(hw, short, (crop, crop))
        use = crops if hw == (224, 224) else [(I.random_image(7, 5, 3, seed=1), 0), (I.ramp(10, 9, 3), 1), (I.random_image(40, 30, 1, seed=2), 0)]
        got = _device(eng, use, hw, tables=tables)
        assert got.shape == (len(use), crop, crop, 3)
        assert np.array_equal(got, intake.host_chain_bytes(use, hw, tables))


def test_libms_weights_stay_within_a_level_where_numpy_is_not_stated(eng):
    """Without xfr_intake_set_kernels the library takes libm's exp under numpy's summation: the weights may differ from numpy's in the last bit, a
    byte then only where the value sat within that of an integer."""
    crops = [(I.ramp(300, 300, 3), 0), (I.random_image(421, 333, 3, seed=3), 1)]
    src, table = intake.pack(crops)
    eng.intake_set_kernels([], [], np.zeros((0, intake.MAX_RADIUS + 1)))
    got = eng.intake_u8(src, table, (224, 224)).cpu().numpy().astype(int)
    want = np.stack([intake.host_bytes(u, (224, 224), head) for u, head in crops]).astype(int)
    print('libm weights: %d of %d bytes differ' % (int((got != want).sum()), want.size))
    assert np.abs(got - want).max() <= 1 and (got != want).mean() < 1e-3


def test_refusals_launch_nothing(eng):
    lib, h = eng.lib, eng._h
    src = torch.full((4096,), 7, dtype=torch.uint8, device=eng.device)
    out = torch.full((2 * 8 * 8 * 3,), 201, dtype=torch.uint8, device=eng.device)
    tabs = pil_bilinear_tables((8, 8), 6, (4, 4))
    from xfr_amd.engine import _tap_array
    row, col = _tap_array(tabs[0]), _tap_array(tabs[1])

    def call(text, fn=None, e=h, s=src.data_ptr(), nbytes=4096, items=((0, 16, 16, 48, 3, 0),), n=None, H=8, W=8, row=None, col=None, fh=4, fw=4,
             o=out.data_ptr()):
        table = None if items is None else (intake.Item * len(items))(*[intake.Item(*it) for it in items])
        n = len(items) if n is None else n
        for f in ((lib.xfr_intake_u8, lib.xfr_intake_u8_host) if fn is None else (fn,)):
            hs = np.full(4096, 7, np.uint8)
            sp = s if (f is lib.xfr_intake_u8 or not s) else hs.ctypes.data
            st = f(e, sp, nbytes, ctypes.cast(table, ctypes.c_void_p) if table is not None else None, n, H, W, row, col, fh, fw, o, None)
            assert st == _lib.XFR_INVALID_ARG, (text, st)
            assert text in lib.xfr_last_error(), lib.xfr_last_error()

    call(b'null engine', e=None)
    call(b'null source', s=None)
    call(b'null source', o=None)
    call(b'null source', items=None, n=1)
    call(b'0 items', n=0)
    call(b'%d items' % (_lib.INTAKE_MAX_ITEMS + 1), n=_lib.INTAKE_MAX_ITEMS + 1)
    call(b'2 channels', items=((0, 16, 16, 32, 2, 0),))
    call(b'head 2', items=((0, 16, 16, 48, 3, 2),))
    call(b'is 0 x 16', items=((0, 0, 16, 48, 3, 0),))
    call(b'is 16 x 4097', items=((0, 16, 4097, 3 * 4097, 3, 0),), nbytes=1 << 30)
    call(b'output of 8 x 4097', W=4097)
    call(b'row stride of 47', items=((0, 16, 16, 47, 3, 0),))
    call(b'reads bytes [3329, 4097)', items=((3329, 16, 16, 48, 3, 0),))
    call(b'reads bytes [-1,', items=((-1, 16, 16, 48, 3, 0),))
    call(b'item 1 reads bytes', items=((0, 16, 16, 48, 3, 0), (4000, 16, 16, 48, 3, 0)))
    call(b'radius 130', items=((0, 1, 4096, 4096, 1, 0),), H=1, W=62)
    call(b'one tap table without the other', row=row)
    call(b'final size of 0 x 4', row=row, col=col, fh=0)
    bad = _tap_array(tabs[0])
    bad[1].count = 9
    call(b'intake_u8: row table entry 1 has count 9', row=bad, col=col)
    bad = _tap_array(tabs[1])
    bad[2].first = 7
    call(b'intake_u8: column table entry 2 reads', row=row, col=bad)
    call(b'the output overlaps the source', fn=lib.xfr_intake_u8, o=src.data_ptr() + 100)
    torch.cuda.synchronize()
    assert bool((out == 201).all()) and bool((src == 7).all())
    assert lib.xfr_intake_set_kernels(h, None, None, None, 1) == _lib.XFR_INVALID_ARG and b'null array' in lib.xfr_last_error()
    one = (ctypes.c_double * 1)(0.5)
    rad = (ctypes.c_int32 * 1)(65)
    wts = (ctypes.c_double * 65)()
    assert lib.xfr_intake_set_kernels(h, one, rad, wts, 1) == _lib.XFR_INVALID_ARG and b'radius 65' in lib.xfr_last_error()


def _pictures():
    return [I.random_image(224, 224, 3, seed=31), I.ramp(300, 300, 3), I.random_image(96, 131, 3, seed=32), I.ramp(223, 225, 3), I.random_image(160, 160, 3, seed=33)]


@pytest.mark.parametrize('which', ['mini32', 'lcnn'])
def test_whitebox_intake_feeds_encode_u8(request, which, tmp_path):
    """Whitebox.intake -> encode_u8 against embeddings(..., intake='host') at the same batch split, bit for bit: uint8 arrays (the float32 head),
    files (the float64 head, the centred square), on a sub-mean and on a luminance network."""
    import PIL.Image
    wb = request.getfixturevalue(which)
    old, wb.batch_size = wb.batch_size, 2
    try:
        pics = _pictures()
        fns = []
        for k, p in enumerate(pics):
            fns.append(str(tmp_path / ('p%d.png' % k)))
            PIL.Image.fromarray(p if k != 2 else p[:, :, 0]).save(fns[-1])
        for images in (pics, fns):
            u8 = wb.intake(images)
            side = wb.net.net.in_shape[1]
            assert u8.dtype == torch.uint8 and u8.is_cuda and tuple(u8.shape) == (5, side, side, 3)
            dev = torch.cat([wb.net.encode_u8(b) for b in torch.split(u8, wb.batch_size)]).cpu()
            if images is pics:      # the parent takes H x W x 3 arrays through convert_from_numpy first (WhiteboxBlackBox._vectors)
                host = wb.embeddings([wb.convert_from_numpy(im)[0] for im in images], norm=False)
            else:
                host = wb.embeddings(images, norm=False, intake='host')
            assert torch.equal(dev, torch.from_numpy(host).reshape(dev.shape))
            for mode in ('auto', 'device'):
                assert np.array_equal(wb.embeddings(images, norm=False, intake=mode), host)
        # the gallery encodes of the inpainting-game callers (inpainting_game.encode_images): the same encodings from either intake
        from xfr_amd import inpainting_game as IG
        dev = u8.device
        enc_host = IG.encode_images(wb, pics, dev, wb.batch_size, intake='host')
        for mode in ('auto', 'device'):
            assert torch.equal(IG.encode_images(wb, pics, dev, wb.batch_size, intake=mode), enc_host)
        floats = [p.astype(float) / 255 for p in pics[:2]]
        with pytest.raises(intake.IntakeRefused):
            IG.encode_images(wb, floats, dev, 1, intake='device')
        with pytest.raises(intake.IntakeRefused):
            wb.embeddings(floats, intake='device')
        with pytest.raises(ValueError):
            wb.embeddings(fns, intake='gpu')
        assert wb.embeddings(floats, norm=False).shape[0] == 2      # 'auto' falls back to the host chain
    finally:
        wb.batch_size = old
