"""STRise behind the generator's black box, the host side (no GPU): scipy's zoom restated to the bit (mask_law_scipy), PIL's bilinear resize restated
in integers (pil_bilinear_tables), WhiteboxBlackBox's conversion chain against the real reference's run (tests/golden/golden_strise_wb.npz,
make_golden_strise_wb.py), the routing between the native sweep and the callable, and the new C-ABI symbols with the ABI version unchanged.
Whitebox.embeddings has no CPU path (the engine is the only compute path), so the callable itself is compared on the GPU (test_gpu_strise_wb.py)."""
import ctypes
import os
import re
import zlib

import numpy as np
import PIL.Image
import pytest
import scipy.ndimage

from parity_utils import make_backbone
from xfr_amd import _lib, synth
from xfr_amd.models import blackbox as BB
from xfr_amd.models import whitebox as WB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_strise_wb.npz'))
CASES = ('mini/blur', 'mini/gray', 'mini/e40', 'lcnn/blur', 'r50/blur', 'r101/blur')
EX_SYMBOLS = ('xfr_strise_score_ex', 'xfr_strise_combine_ex', 'xfr_strise_debug_masks_ex', 'xfr_strise_debug_masked_probes_ex',
              'xfr_strise_debug_quantized')


def _zoom(grid, H, W, s):
    full = scipy.ndimage.zoom(grid, ((H + s) / float(grid.shape[0]), (W + s) / float(grid.shape[1])), order=1, mode='mirror', grid_mode=True)
    assert full.shape == (H + s, W + s)
    return full


def _grids(H, W, s, n, seed):
    gh, gw = -(-H // s), -(-W // s)
    rng = np.random.RandomState(seed)
    for i in range(n):
        grid = np.ones(gh * gw)
        grid[rng.choice(gh * gw, min(1 + 3 * i, gh * gw), replace=False)] = 0.0
        if i == 0:
            grid[[0, gw - 1, gh * gw - 1]] = 0.0      # corners: the reflected coordinate and the folded tap
        yield grid.reshape(gh, gw)


@pytest.mark.parametrize('H,W,s,n', [(7, 9, 3, 3), (37, 53, 5, 3), (224, 224, 12, 2)])
def test_mask_law_scipy_is_scipy_zoom_bit_for_bit(H, W, s, n):
    """Every shift of every grid: == on float64 arrays, no tolerance."""
    for grid in _grids(H, W, s, n, seed=H):
        full = _zoom(grid, H, W, s)
        for x in range(s):
            for y in range(s):
                got = BB.mask_law_scipy(grid, (H, W), s, (x, y))
                assert got.dtype == np.float64 and np.array_equal(got, full[x:x + H, y:y + W]), (x, y)


def test_mask_law_scipy_with_a_single_cell_axis():
    """g == 1 along both axes, and along one."""
    for H, W, s, grid in ((3, 3, 3, np.zeros((1, 1))), (3, 3, 3, np.ones((1, 1))), (4, 9, 4, np.array([[1.0, 0.0, 1.0]]))):
        full = _zoom(grid, H, W, s)
        for x in range(s):
            for y in range(s):
                assert np.array_equal(BB.mask_law_scipy(grid, (H, W), s, (x, y)), full[x:x + H, y:y + W])


def test_exact_law_is_not_the_closed_form_where_it_matters():
    """The finding behind the exact law: where no drawn cell is near, scipy returns 1 - 2**-53 (or 1 - 2**-52) at many pixels and the closed form 1."""
    grid = next(_grids(224, 224, 12, 1, seed=5))
    a, b = BB.mask_law(grid, (224, 224), 12, (3, 7)), BB.mask_law_scipy(grid, (224, 224), 12, (3, 7))
    differ = a != b
    assert differ.any() and np.abs(a - b).max() <= 2.0 ** -52
    below = b[differ & (a == 1.0)] < 1.0                  # one or two ulps below 1: a uint8 level wherever the fill lies below the probe
    assert below.sum() > 100 and (b[differ & (a == 1.0)] >= 1.0 - 2.0 ** -52).all()


@pytest.mark.parametrize('h,w', [(224, 224), (131, 150), (100, 100)])
def test_pil_tables_are_pil_bit_for_bit(h, w):
    """Resize(144) + CenterCrop(128): a downscale with ksize 5, a non-square probe, an upscale with ksize 3; a random and a smooth image each."""
    rng = np.random.RandomState(h)
    smooth = synth.synth_smooth_images(1, (3, h, w), seed=3)[0].permute(1, 2, 0).numpy().astype(np.uint8)
    row_tab, col_tab = BB.pil_bilinear_tables((h, w), 144, (128, 128))
    assert row_tab['coef'].shape == (128, 5 if h == 224 else 3) and (row_tab['coef'] >= 0).all() and (col_tab['coef'] >= 0).all()
    assert row_tab['count'].max() <= BB.STRISE_MAX_TAPS and row_tab['count'].min() >= 1
    nw, nh = (144, int(144 * h / w)) if w <= h else (int(144 * w / h), 144)
    left, top = int(round((nw - 128) / 2.0)), int(round((nh - 128) / 2.0))
    for img in (rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8), smooth):
        want = np.asarray(PIL.Image.fromarray(img).resize((nw, nh), PIL.Image.BILINEAR).crop((left, top, left + 128, top + 128)))
        assert np.array_equal(BB.apply_pil_tables(img, row_tab, col_tab), want)


def test_pil_tables_equal_the_networks_own_preprocess():
    """lightcnn_preprocess (Resize(144), CenterCrop(128), rgb2gray) of a uint8 image == rgb2gray of the tables' image, as float32 tensors."""
    from xfr_amd.models.lightcnn import lightcnn_preprocess, prepare_lightCNN_image
    img = np.random.RandomState(1).randint(0, 256, size=(224, 224, 3)).astype(np.uint8)
    row_tab, col_tab = BB.pil_bilinear_tables((224, 224), 144, (128, 128))
    got = prepare_lightCNN_image(BB.apply_pil_tables(img, row_tab, col_tab))
    assert np.array_equal(got.numpy(), lightcnn_preprocess()(PIL.Image.fromarray(img)).numpy())


def _images():
    return [synth.synth_smooth_images(1, (3, 224, 224), seed=s)[0].permute(1, 2, 0).numpy().astype(np.uint8) for s in range(1, 8)]


def _host_whitebox(arch):
    bb, _ = make_backbone(arch if arch != 'stresnet101' else 'stresnet_mini', seed=0, num_classes={'lightcnn29v2': 10, 'resnet50_128': None}.get(arch, 5))
    wbn = {'lightcnn29v2': WB.WhiteboxLightCNN, 'resnet50_128': WB.Whitebox_resnet50_128}.get(arch, WB.WhiteboxSTResnet)(bb)
    return WB.Whitebox(wbn)


def _fill(case, probe):
    st = BB.STRise(probe=probe, refs=[probe], black_box_fn=lambda p, g: None, mask_fill_type=str(GOLD[case + '/fill']))
    st.apply_masks()
    return st.fill_image


def _masked(case, probe, fill, k):
    g = -(-224 // 12)
    grid = np.ones(g * g)
    grid[GOLD[case + '/mask_cells'][k]] = 0.0
    m = BB.mask_law_scipy(grid.reshape(g, g), (224, 224), 12, GOLD[case + '/mask_shifts'][k])[..., None]
    return m * probe + (1.0 - m) * fill


def _gold_tensor(case, q_gold):
    """The reference's fp32 network input of masks 0-1: stored as it is for Light-CNN, as its per-channel table of levels for the sub-mean networks."""
    if case + '/tensor' in GOLD.files:
        return GOLD[case + '/tensor']
    lut = GOLD[case + '/tensor_lut']
    t = np.stack([lut[c][q_gold[:2, :, :, c]] for c in range(3)], axis=1)
    assert not np.isnan(t).any()
    return t


@pytest.mark.parametrize('case', CASES)
def test_conversion_chain_is_the_references(case):
    """convert_from_numpy on the host masks of mask_law_scipy: the uint8 image handed to preprocess equals the fixture's q (masks 0-3 as arrays, every
    mask by CRC32) and the tensor equals the fixture's for masks 0-1, bit for bit.  (The ResNet-101 preprocessing does not depend on the weights:
    the mini network stands in for it.)"""
    wb = _host_whitebox(str(GOLD[case + '/arch']))
    probe = _images()[0]
    fill = _fill(case, probe)
    seen = []
    inner = wb.net.preprocess
    wb.net.preprocess = lambda im: (seen.append(np.array(im)), inner(im))[1]
    n = int(GOLD[case + '/num_masks'])
    tens = [wb.convert_from_numpy(_masked(case, probe, fill, k)) for k in range(n)]
    q_gold = probe[None] + GOLD[case + '/dq']             # uint8 arithmetic: the fixture stores q minus the probe modulo 256
    assert q_gold.dtype == np.uint8 and np.array_equal(np.stack(seen[:4]), q_gold)
    assert [zlib.crc32(q.tobytes()) for q in seen] == list(GOLD[case + '/q_crc'])
    got = np.concatenate([t.numpy() for t in tens[:2]])
    assert got.dtype == np.float32 and np.array_equal(got, _gold_tensor(case, q_gold))
    # the unmasked probe passes the chain unchanged: image zero of the sweep is the probe itself
    del seen[:]
    wb.convert_from_numpy(probe)
    assert np.array_equal(seen[0], probe)


@pytest.mark.parametrize('case', CASES)
def test_fixture_condition_holds(case):
    s32, s64 = GOLD[case + '/scores32'], GOLD[case + '/scores64']
    top = np.abs(s64).max()
    r = np.abs(s32 - s64).max() / top
    assert np.abs(s64).min() >= 10 * r * top and np.array_equal(np.sign(s32), np.sign(s64))
    assert int(GOLD[case + '/int_near']) > 0      # the last-bit effect is in every case: the exact law is exercised
    # ... and it is a last-bit effect: whatever quantises within 1e-9 of an integer is within two ulps of [128, 256) of it
    assert 0 < float(GOLD[case + '/int_near_dist']) <= 2.0 ** -44


class _FakeEngine(object):
    max_batch = 4

    def __init__(self):
        self.calls = []

    def strise_score(self, probe, fill, cells, shifts, grid, scale, refs, gal, enc, **kw):
        import torch
        self.calls.append(kw)
        return torch.arange(len(cells), dtype=torch.float64) - 1.5, torch.zeros(len(refs) + len(gal), dtype=torch.float64)


def _routed(monkeypatch, probe, arch='stresnet_mini', fill='blur', spec='keep', tables='keep', in_shape=None):
    """score_masks with the engines faked: -> (score_route, the keyword arguments the native sweep got or None)."""
    import torch
    wb = _host_whitebox(arch)
    box = BB.WhiteboxBlackBox(wb)
    eng = _FakeEngine()
    monkeypatch.setattr(wb, '_engine', lambda n=1: eng)
    monkeypatch.setattr(wb.net, '_mark', lambda name: 7)
    monkeypatch.setattr(box, 'embed_raw', lambda images: torch.zeros(len(images), 4))
    if spec != 'keep':
        monkeypatch.setattr(wb.net, 'u8_preprocess_spec', lambda: spec)
    if tables != 'keep':
        monkeypatch.setattr(box, 'resample_tables', lambda hw: tables)
    if in_shape is not None:
        monkeypatch.setattr(wb.net.net, 'in_shape', in_shape, raising=False)
    st = BB.STRise(probe=probe, refs=[probe], gallery=[probe], black_box_fn=box, num_masks=6, num_mask_elements=2, mask_fill_type=fill)
    st.mask_cells = np.array([[0, 1]] * 6, dtype=np.int32)
    st.mask_shifts = np.zeros((6, 2), dtype=np.int32)
    st.apply_masks()
    host = []
    monkeypatch.setattr(BB.WhiteboxBlackBox, '__call__', lambda self, probes, gallery: (host.append(len(probes)), np.ones((len(probes), len(gallery))))[1])
    monkeypatch.setattr(BB.STRise, '_engine', lambda self: (eng, 7))
    monkeypatch.setattr(BB.STRise, '_masked_batch', lambda self, first, count: np.zeros((count,) + probe.shape))
    st.score_masks()
    assert len(st.mask_scores) == 6
    assert bool(host) == st.score_route.startswith('host')
    return st.score_route, (eng.calls[0] if eng.calls else None)


def test_routing_takes_the_native_sweep_and_falls_back_under_its_conditions(monkeypatch):
    probe = _images()[0]
    route, kw = _routed(monkeypatch, probe)
    assert route == 'device' and kw['quantize'] is True and tuple(kw['probe_shape']) == (224, 224) and kw['tables'] is None
    route, kw = _routed(monkeypatch, probe, arch='lightcnn29v2')
    assert route == 'device' and kw['quantize'] is True and kw['tables'][0]['coef'].shape == (128, 5)
    # 1. a probe that is not 224 x 224
    small = np.ascontiguousarray(probe[:200, :200])
    monkeypatch.setattr(BB, 'center_crop', lambda p, convert_uint8=True: p)
    route, kw = _routed(monkeypatch, small)
    assert route.startswith('host') and 'not 224 x 224' in route and kw is None
    # 2. min(probe, fill) below 2 everywhere: the / 255 of convert_from_numpy is conditional
    dark = np.minimum(probe, 1)
    route, kw = _routed(monkeypatch, dark, fill='gray')
    assert route.startswith('host') and 'below 2' in route and kw is None
    route, kw = _routed(monkeypatch, probe, fill='gray')      # gray fill 0.5 under a bright probe: min is 0.5 < 2 as well
    assert route.startswith('host') and 'below 2' in route
    # 3. a table with more than 8 taps
    first, count, coef = BB.pil_bilinear_axis(224, 32)
    assert count.max() > BB.STRISE_MAX_TAPS
    big = dict(first=first, count=count, coef=coef)
    route, kw = _routed(monkeypatch, probe, arch='lightcnn29v2', tables=(big, big))
    assert route.startswith('host') and 'more than 8 taps' in route and kw is None
    # 4. a network without u8_preprocess_spec
    route, kw = _routed(monkeypatch, probe, spec=None)
    assert route.startswith('host') and 'u8_preprocess_spec' in route and kw is None
    # and a fifth, of the device path's own: a sub-mean network whose input is not the 224 x 224 that convert_from_numpy produces (the C call
    # would refuse it)
    route, kw = _routed(monkeypatch, probe, in_shape=(3, 112, 112))
    assert route.startswith('host') and 'network input is not 224 x 224' in route and kw is None


def test_blackbox_is_a_plain_callable_and_refuses_other_networks():
    with pytest.raises(ValueError, match='xfr_amd Whitebox'):
        BB.WhiteboxBlackBox(object())
    box = BB.WhiteboxBlackBox(_host_whitebox('stresnet_mini'))
    assert callable(box) and box.resample_tables((224, 224)) is None
    st = BB.STRise(probe=_images()[0], refs=[_images()[1]], black_box_fn=box)
    assert st.black_box is None and st.black_box_fn is box


def test_ex_symbols_declared_bound_exported_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, 'include', 'xfr_amd.h')).read()
    declared = set(re.findall(r'xfr_status\s+XFR_EX\s+(xfr_strise_\w+)\s*\(', hdr))
    assert declared == set(EX_SYMBOLS)
    bound = [n for n, _, _ in _lib.SYMBOLS]
    lib = _lib.load()
    for name in EX_SYMBOLS:
        assert name in bound and hasattr(lib, name)
    assert '#define XFR_AMD_ABI_VERSION 7' in hdr and _lib.ABI_VERSION == 7 and lib.xfr_abi_version() == 7
    assert '#define XFR_STRISE_MAX_TAPS %d' % _lib.STRISE_MAX_TAPS in hdr and ctypes.sizeof(_lib.StriseTap) == 8 + 4 * _lib.STRISE_MAX_TAPS
    for cite in ('generate_inpaintinggame_bb_saliency_maps_multigpu.py:69-113', 'generate_blackbox_saliency.py:48-73', 'whitebox.py:787-806',
                 'lightcnn.py:19-31'):
        assert cite in hdr
    geom = _lib.StriseGeometry(19, 19, 12, 1)
    opt = _lib.StriseOptions(struct_size=ctypes.sizeof(_lib.StriseOptions), probe_h=224, probe_w=224, quantize=1)
    st = lib.xfr_strise_combine_ex(None, None, 1, None, None, 1, ctypes.byref(geom), 1, None, ctypes.byref(opt), None)
    assert st == _lib.XFR_INVALID_ARG and b'null engine' in lib.xfr_last_error()
