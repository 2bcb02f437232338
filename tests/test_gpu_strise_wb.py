"""GPU tests of the native STRise sweep behind the generator's black box (include/xfr_amd.h: xfr_strise_*_ex, xfr_strise_debug_quantized;
xfr_amd.models.blackbox.WhiteboxBlackBox) against the real reference's CPU run of the eval script's bb_fn (tests/golden/golden_strise_wb.npz,
make_golden_strise_wb.py), against scipy's zoom and against PIL.

Bars (none of them taken from the code under test):
  masks          == scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True) as restated by mask_law_scipy (test_strise_wb_host.py pins that
                 restatement to scipy bit for bit): float64 arrays, no tolerance;
  q              == the reference's uint8 images: masks 0-3 as arrays, every mask by CRC32, and == numpy's chain on mask_law_scipy; no level and no
                 mask is left out;
  network input  max|d| == 0 against the reference's fp32 tensors, for the three preprocessings;
  scores         max|gpu - ref64| / max|ref64| <= 4 r, r = max|ref32 - ref64| / max|ref64| read from the fixture (the bar of test_gpu_strise.py);
  map            <= 4 x the fixture's ref32-to-ref64 map distance given the engine's own scores (the bar of test_gpu_strise.py), plus 2**-25: map64
                 is stored as float32, half an ulp of [0.5, 1) -- in the 40-element case the reference's own distance (4.9e-12) lies below it;
  sweep vs hook  the sweep's scores against numpy's float64 evaluation of blackbox.py:385-394 on the encodings of the parity hook's batches: 1e-12
                 (two float64 summation orders over D <= 512 terms of magnitude <= 2: 512 x 2 x 2**-53 = 1.1e-13, and a square root)."""
import functools
import zlib

import numpy as np
import PIL.Image
import pytest
import torch

import probe_scoring_utils as U
from parity_utils import make_backbone
from probe_scoring_utils import images, lcnn, mini32, mini48, r50      # noqa: F401 (fixtures)
from xfr_amd import synth
from xfr_amd.models import blackbox as BB
from xfr_amd.models.lightcnn import prepare_lightCNN_image

pytestmark = pytest.mark.gpu
GOLD = U.gold('strise_wb')
CASES = ('mini/blur', 'mini/gray', 'mini/e40', 'lcnn/blur', 'r50/blur', 'r101/blur')
SCALE = 12
_whitebox, _score_error = U.whitebox, functools.partial(U.score_error, GOLD)


@pytest.fixture(scope='module')
def fills(images):
    """{fill type: the fill image}, as STRise computes it on the host."""
    out = {}
    for fill in ('blur', 'gray'):
        st = BB.STRise(probe=images[0], refs=[images[1]], black_box_fn=lambda p, g: None, mask_fill_type=fill)
        st.apply_masks()
        out[fill] = st.fill_image
    return out


def _case(case, fills):
    return GOLD[case + '/mask_cells'], GOLD[case + '/mask_shifts'], fills[str(GOLD[case + '/fill'])]


def _host_q(probe, fill, cells, shifts, scale=SCALE):
    """numpy's chain: mask_law_scipy, blackbox.py:343, whitebox.py:794-795,803."""
    h, w = probe.shape[0:2]
    gh, gw = -(-h // scale), -(-w // scale)
    out = np.empty((len(cells),) + probe.shape, dtype=np.uint8)
    for k in range(len(cells)):
        grid = np.ones(gh * gw)
        grid[cells[k]] = 0.0
        m = BB.mask_law_scipy(grid.reshape(gh, gw), (h, w), scale, shifts[k])[..., None]
        out[k] = (((m * probe + (1.0 - m) * fill) / 255) * 255).astype(np.uint8)
    return out


def _gold_tensor(case, q_gold):
    if case + '/tensor' in GOLD.files:
        return GOLD[case + '/tensor']
    lut = GOLD[case + '/tensor_lut']
    t = np.stack([lut[c][q_gold[:2, :, :, c]] for c in range(3)], axis=1)
    assert not np.isnan(t).any()
    return t


def _box_for(case, mini48, lcnn, r50):
    return {'lightcnn29v2': lcnn, 'resnet50_128': r50}.get(str(GOLD[case + '/arch']), mini48)


def _native_scores(case, wb, images, fills):
    """xfr_strise_score_ex(quantize = 1) on wb's engine with the fixture's draws -> (scores, orig) as numpy."""
    box = BB.WhiteboxBlackBox(wb)
    cells, shifts, fill = _case(case, fills)
    n_refs, n_gal = int(GOLD[case + '/n_refs']), int(GOLD[case + '/n_gal'])
    refs, gal = box.embed_raw(list(images[1:1 + n_refs])), box.embed_raw(list(images[4:4 + n_gal]))
    eng = wb._engine(wb.batch_size)
    scores, orig = eng.strise_score(torch.from_numpy(images[0]), torch.from_numpy(fill), cells, shifts, (19, 19), SCALE, refs, gal, wb.net._mark('encode'),
                                    probe_shape=(224, 224), quantize=True, tables=box.resample_tables((224, 224)))
    return scores.cpu().numpy(), orig.cpu().numpy()


# ---- masks -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_elem', [1, 40])
@pytest.mark.parametrize('h,w,s', [(7, 9, 3), (37, 53, 5), (128, 128, 12), (224, 224, 12)])
def test_exact_masks_equal_scipy_bit_for_bit(mini48, h, w, s, n_elem):
    """Every shift value occurs; 40 elements where the grid has them, else all cells but one (3 x 3 and 8 x 11 cells)."""
    eng = mini48._engine(48)
    gh, gw = -(-h // s), -(-w // s)
    n_elem = min(n_elem, gh * gw - 1)
    rng = np.random.RandomState(h + n_elem)
    n = 2 * s
    cells = np.stack([rng.choice(gh * gw, n_elem, replace=False) for _ in range(n)]).astype(np.int32)
    cells[0, 0], cells[1, 0] = (0, gh * gw - 1) if n_elem == 1 else (cells[0, 0], cells[1, 0])      # corners: reflected coordinate, folded tap
    shifts = np.stack([np.arange(n) % s, (np.arange(n) * 5 + 1) % s], axis=1).astype(np.int32)
    got = eng.strise_masks(cells, shifts, (gh, gw), s, probe_shape=(h, w), exact=True).cpu().numpy()
    assert got.shape == (n, h, w) and got.dtype == np.float64
    for k in range(n):
        grid = np.ones(gh * gw)
        grid[cells[k]] = 0.0
        assert np.array_equal(got[k], BB.mask_law_scipy(grid.reshape(gh, gw), (h, w), s, shifts[k])), (k, cells[k], shifts[k])
    closed = eng.strise_masks(cells, shifts, (gh, gw), s, probe_shape=(h, w)).cpu().numpy()
    assert np.abs(closed - got).max() <= 1e-12


# ---- q ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_q_is_the_references_for_every_mask(mini48, images, fills, case):
    eng = mini48._engine(48)
    cells, shifts, fill = _case(case, fills)
    n = len(cells)
    q = eng.strise_quantized(torch.from_numpy(images[0]), torch.from_numpy(fill), cells, shifts, (19, 19), SCALE).cpu().numpy()
    assert q.shape == (n, 224, 224, 3) and q.dtype == np.uint8
    q_gold = images[0][None] + GOLD[case + '/dq']          # uint8 arithmetic: the fixture stores q minus the probe modulo 256
    assert np.array_equal(q[:4], q_gold)
    assert [zlib.crc32(q[k].tobytes()) for k in range(n)] == list(GOLD[case + '/q_crc'])
    assert np.array_equal(q, _host_q(images[0], fill, cells, shifts))


@pytest.mark.parametrize('h,w,s', [(37, 53, 5), (30, 30, 16), (13, 7, 3)])
def test_q_on_probes_whose_width_is_no_multiple_of_four(mini48, h, w, s):
    """The scalar tail of strise_quant_kernel (W % 4 = 1, 2, 3: the last thread of a row holds fewer than four pixels) at sizes other than 224, several
    workgroups per image at 37 x 53: q of image zero, of every mask and of a padding row against numpy's chain."""
    rng = np.random.RandomState(w)
    probe = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    fill = rng.uniform(0.0, 255.0, size=(h, w, 3))
    gh, gw = -(-h // s), -(-w // s)
    n = 2 * s
    cells = np.stack([rng.choice(gh * gw, min(3, gh * gw - 1), replace=False) for _ in range(n)]).astype(np.int32)
    shifts = np.stack([np.arange(n) % s, (np.arange(n) * 3 + 2) % s], axis=1).astype(np.int32)
    q = mini48._engine(48).strise_quantized(torch.from_numpy(probe), torch.from_numpy(fill), cells, shifts, (gh, gw), s, first=-1, count=n + 2,
                                            probe_shape=(h, w)).cpu().numpy()
    assert q.shape == (n + 2, h, w, 3) and np.array_equal(q[0], probe) and np.array_equal(q[n + 1], probe)
    want = _host_q(probe, fill, cells, shifts, scale=s)
    assert np.array_equal(q[1:n + 1], want) and (want != probe[None]).any()


def test_image_zero_and_padding_rows_are_the_probe(mini48, lcnn, images, fills):
    """Rows -1 (image zero of the sweep) and n_masks .. of the image list bypass the mask: q = probe, and the network input is the probe's."""
    case = 'mini/blur'
    cells, shifts, fill = _case(case, fills)
    probe, n = torch.from_numpy(images[0]), len(cells)
    eng = mini48._engine(48)
    q = eng.strise_quantized(probe, torch.from_numpy(fill), cells, shifts, (19, 19), SCALE, first=-1, count=2).cpu().numpy()
    assert np.array_equal(q[0], images[0]) and np.array_equal(q[1], _host_q(images[0], fill, cells[:1], shifts[:1])[0])
    q = eng.strise_quantized(probe, torch.from_numpy(fill), cells, shifts, (19, 19), SCALE, first=n - 1, count=4).cpu().numpy()
    assert not np.array_equal(q[0], images[0]) and all(np.array_equal(q[i], images[0]) for i in (1, 2, 3))
    x = eng.strise_masked_probes(probe, torch.from_numpy(fill), cells, shifts, (19, 19), SCALE, first=n - 1, count=3, probe_shape=(224, 224),
                                 quantize=True).cpu().numpy()
    want = mini48.convert_from_numpy(images[0]).numpy()
    assert np.array_equal(x[1:], np.concatenate([want, want]))
    box = BB.WhiteboxBlackBox(lcnn)
    x = lcnn._engine(8).strise_masked_probes(probe, torch.from_numpy(fill), cells, shifts, (19, 19), SCALE, first=-1, count=1, probe_shape=(224, 224),
                                            quantize=True, tables=box.resample_tables((224, 224))).cpu().numpy()
    assert np.array_equal(x, lcnn.convert_from_numpy(images[0]).numpy())
    # an all-ones grid under the exact law is NOT the probe: this is why those rows carry no mask
    ones = eng.strise_masks(np.array([[0]], dtype=np.int32), np.array([[3, 7]], dtype=np.int32), (19, 19), SCALE, probe_shape=(224, 224), exact=True)
    assert (ones.cpu().numpy()[0][100:, 100:] != 1.0).any()


# ---- network input ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['mini/blur', 'mini/gray', 'mini/e40', 'lcnn/blur', 'r50/blur'])
def test_network_input_equals_the_references_tensor(mini48, lcnn, r50, images, fills, case):
    wb = _box_for(case, mini48, lcnn, r50)
    cells, shifts, fill = _case(case, fills)
    tables = BB.WhiteboxBlackBox(wb).resample_tables((224, 224))
    got = wb._engine(wb.batch_size).strise_masked_probes(torch.from_numpy(images[0]), torch.from_numpy(fill), cells, shifts, (19, 19), SCALE, first=0, count=2,
                                                         probe_shape=(224, 224), quantize=True, tables=tables).cpu().numpy()
    want = _gold_tensor(case, images[0][None] + GOLD[case + '/dq'])
    d = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    print('%s network input: max|d| = %.3e' % (case, d))
    assert got.shape == want.shape and got.dtype == np.float32 and d == 0


@pytest.mark.parametrize('h,w', [(131, 150), (100, 100)])
def test_luminance_path_on_other_probe_sizes(lcnn, h, w):
    """W % 4 != 0, a non-square probe, the upscale's ksize 3 and windows clipped at both edges: each network input equals PIL's
    Resize(144) + CenterCrop(128) of numpy's q followed by the host luminance, bit for bit."""
    rng = np.random.RandomState(h)
    probe = synth.synth_smooth_images(1, (3, h, w), seed=9)[0].permute(1, 2, 0).numpy().astype(np.uint8)
    fill = np.ascontiguousarray(probe[::-1, ::-1].astype(np.float64) * 0.75 + 3.0)
    gh, gw = -(-h // SCALE), -(-w // SCALE)
    cells = np.stack([rng.choice(gh * gw, 3, replace=False) for _ in range(6)]).astype(np.int32)
    shifts = rng.randint(0, SCALE, size=(6, 2)).astype(np.int32)
    tables = BB.pil_bilinear_tables((h, w), 144, (128, 128))
    got = lcnn._engine(8).strise_masked_probes(torch.from_numpy(probe), torch.from_numpy(fill), cells, shifts, (gh, gw), SCALE, first=-1, count=7,
                                              probe_shape=(h, w), quantize=True, tables=tables).cpu().numpy()
    q = np.concatenate([probe[None], _host_q(probe, fill, cells, shifts)])
    nw, nh = (144, int(144 * h / w)) if w <= h else (int(144 * w / h), 144)
    left, top = int(round((nw - 128) / 2.0)), int(round((nh - 128) / 2.0))
    for k in range(7):
        im = PIL.Image.fromarray(q[k]).resize((nw, nh), PIL.Image.BILINEAR).crop((left, top, left + 128, top + 128))
        assert np.array_equal(got[k], prepare_lightCNN_image(im).numpy()[0]), k
    assert (q[1:] != probe[None]).any()


# ---- scores and map --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['mini/blur', 'mini/gray', 'mini/e40', 'lcnn/blur', 'r50/blur'])
def test_scores_and_map(mini48, lcnn, r50, images, fills, case):
    """lcnn/blur: 20 masks + the probe at batch 8, a three-batch sweep; r50/blur: 13 images at batch 4."""
    wb = _box_for(case, mini48, lcnn, r50)
    scores, orig = _native_scores(case, wb, images, fills)
    err, r = _score_error(case, scores)
    print('%s scores: %.3e (r = %.3e, bar %.3e)' % (case, err, r, 4 * r))
    assert scores.shape == (int(GOLD[case + '/num_masks']),) and scores.dtype == np.float64
    assert err <= 4 * r
    assert np.abs(orig - GOLD[case + '/orig64']).max() <= 1e-4
    sel = scores >= np.percentile(scores[scores > 0], 0)
    assert np.array_equal(sel, GOLD[case + '/scores64'] > 0)
    cells, shifts, _ = _case(case, fills)
    sal = wb._engine(wb.batch_size).strise_combine(np.where(sel, scores, 0.0), int(sel.sum()), cells, shifts, (19, 19), SCALE, 1,
                                                   probe_shape=(224, 224)).cpu().numpy()
    d, dist = np.abs(sal - GOLD[case + '/map64']).max(), float(GOLD[case + '/map_dist'])
    print('%s map from the engine\'s scores: %.3e (ref32 vs ref64 %.3e)' % (case, d, dist))
    assert sal.shape == (224, 224) and d <= 4 * dist + 2.0 ** -25


def test_scores_resnet101(gpu_device, images, fills):
    case = 'r101/blur'
    wb = _whitebox('stresnet101', 32, gpu_device, 65359)
    scores, _ = _native_scores(case, wb, images, fills)
    err, r = _score_error(case, scores)
    print('%s scores: %.3e (r = %.3e, bar %.3e)' % (case, err, r, 4 * r))
    assert err <= 4 * r
    sel = scores >= np.percentile(scores[scores > 0], 0)
    assert np.array_equal(sel, GOLD[case + '/scores64'] > 0)
    cells, shifts, _ = _case(case, fills)
    sal = wb._engine(wb.batch_size).strise_combine(np.where(sel, scores, 0.0), int(sel.sum()), cells, shifts, (19, 19), SCALE, 1,
                                                   probe_shape=(224, 224)).cpu().numpy()
    d, dist = np.abs(sal - GOLD[case + '/map64']).max(), float(GOLD[case + '/map_dist'])
    print('%s map from the engine\'s scores: %.3e (ref32 vs ref64 %.3e)' % (case, d, dist))
    assert d <= 4 * dist + 2.0 ** -25
    wb.net._engine.close()


def test_partial_last_batch_and_the_hooks_forward_batch_by_batch(mini32, images, fills):
    """48 masks + the probe at batch 32: two batches, 15 padding rows.  The sweep holds the score bar, and its scores are what blackbox.py:385-394
    gives in float64 on the encodings of the parity hook's batches (rows -1 .. 30 and 31 .. 62 of the image list)."""
    case = 'mini/blur'
    scores, orig = _native_scores(case, mini32, images, fills)
    err, r = _score_error(case, scores)
    print('%s batch 32 scores: %.3e (bar %.3e)' % (case, err, 4 * r))
    assert err <= 4 * r
    cells, shifts, fill = _case(case, fills)
    eng, enc = mini32._engine(32), mini32.net._mark('encode')
    box = BB.WhiteboxBlackBox(mini32)
    emb = []
    for first in (-1, 31):
        x = eng.strise_masked_probes(torch.from_numpy(images[0]), torch.from_numpy(fill), cells, shifts, (19, 19), SCALE, first=first, count=32,
                                     probe_shape=(224, 224), quantize=True)
        emb.append(eng.forward(x, enc).reshape(32, -1).double().cpu().numpy())
    emb = np.concatenate(emb)[:49]
    refs, gal = box.embed_raw(list(images[1:4])).double().numpy(), box.embed_raw(list(images[4:7])).double().numpy()
    sim_r, sim_g = BB.l2_similarity(emb, refs), BB.l2_similarity(emb, gal)
    want = np.mean((sim_r[:1] - sim_r[1:]) - (sim_g[:1] - sim_g[1:]), axis=1)
    d = np.abs(scores - want).max()
    print('sweep against the hook\'s forward: max|d| = %.3e' % d)
    assert d <= 1e-12
    assert np.abs(orig - np.concatenate([sim_r[0], sim_g[0]])).max() <= 1e-12


# ---- the callable and the drop-in class ------------------------------------------------------------------------------------------------
def test_callable_is_the_fixtures_bb_fn(mini48, images):
    """WhiteboxBlackBox.__call__ on the host path: the unmasked probe's scores against the fixture's fp32 run, within the forward's tolerance
    (1e-4 of a similarity in [0, 1], the bar test_gpu_strise.py holds a lone encode to)."""
    box = BB.WhiteboxBlackBox(mini48)
    got = np.concatenate([box([images[0]], list(images[1:4])).ravel(), box([images[0]], list(images[4:7])).ravel()])
    assert np.abs(got - GOLD['mini/blur/orig32']).max() <= 1e-4


def test_evaluate_end_to_end_on_lightcnn_with_the_mini_prior(mini48, lcnn, images):
    """STRise(black_box_fn=WhiteboxBlackBox(Light-CNN)).evaluate() with the prior from the mini ResNet: the native route is taken, the scores are the
    callable's own (the host path of the same class) within the score bar's r of the fixture's Light-CNN case, and run_blackbox_rise returns the map."""
    from xfr_amd.inpainting_game import run_blackbox_rise
    box = BB.WhiteboxBlackBox(lcnn)
    st = BB.STRise(probe=images[0], refs=list(images[1:3]), gallery=list(images[4:6]), black_box_fn=box, num_masks=20, num_mask_elements=2, net=mini48)
    np.random.seed(5)
    st.evaluate()
    assert st.score_route == 'device' and st.mask_scores.shape == (20,) and np.isfinite(st.mask_scores).all()
    assert st.saliency_map.shape == (224, 224) and st.saliency_map.min() == 0.0 and st.saliency_map.max() == 1.0
    # the same masks through the callable on the host: every masked probe as a float64 array through convert_from_numpy
    g = 19
    masked = []
    for k in range(20):
        grid = np.ones(g * g)
        grid[st.mask_cells[k]] = 0.0
        m = BB.mask_law_scipy(grid.reshape(g, g), (224, 224), SCALE, st.mask_shifts[k])[..., None]
        masked.append(m * st.probe + (1.0 - m) * st.fill_image)
    sr, sg = box([st.probe] + masked, st.refs), box([st.probe] + masked, st.gallery)
    want = np.mean((sr[:1] - sr[1:]) - (sg[:1] - sg[1:]), axis=1)
    r = _score_error('lcnn/blur', GOLD['lcnn/blur/scores64'])[1]
    d = np.abs(st.mask_scores - want).max() / np.abs(want).max()
    print('evaluate on Light-CNN: native against the callable %.3e (bar %.3e)' % (d, 4 * r))
    assert d <= 4 * r
    np.random.seed(5)
    sal = run_blackbox_rise(lcnn, images[0], list(images[1:3]), list(images[4:6]), net=mini48, num_masks=20)
    assert np.array_equal(sal, st.saliency_map)


# ---- error paths -----------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch_and_name_the_cause(gpu_device, mini48, lcnn, images, fills):
    cells, shifts, fill = _case('mini/blur', fills)
    probe, fill = torch.from_numpy(images[0]), torch.from_numpy(fill)
    eng, e1 = mini48._engine(48), lcnn._engine(8)
    emb, emb1 = torch.ones((1, 512)), torch.ones((1, 256))
    enc, enc1 = mini48.net._mark('encode'), lcnn.net._mark('encode')
    tables = BB.pil_bilinear_tables((224, 224), 144, (128, 128))

    def lum(**kw):
        args = dict(probe_shape=(224, 224), quantize=True, tables=tables)
        args.update(kw)
        return e1.strise_score(probe, fill, cells, shifts, (19, 19), SCALE, emb1, emb1, enc1, **args)

    def changed(which, i, **kw):
        t = [dict((k, v.copy()) for k, v in tab.items()) for tab in tables]
        for k, v in kw.items():
            t[which][k][i] = v
        return tuple(t)
    # quantize = 1 on an engine without xfr_engine_set_u8_preprocess
    from xfr_amd.engine import Engine
    bare_bb, _ = make_backbone('stresnet_mini', seed=0, num_classes=5)
    bare_bb.to(gpu_device)
    bare = Engine(bare_bb.build_program(), 4, bare_bb.device)
    bare.load_weights(bare_bb.state_dict())
    with pytest.raises(ValueError, match='quantize = 1 needs the engine\'s uint8 preprocessing'):
        bare.strise_score(probe, fill, cells, shifts, (19, 19), SCALE, emb, emb, enc, probe_shape=(224, 224), quantize=True)
    bare.close()
    # a sub-mean engine whose input size is not the probe's
    small = torch.from_numpy(np.ascontiguousarray(images[0][:200, :180]))
    with pytest.raises(ValueError, match='a probe of 200 x 180 for an XFR_U8_SUB_MEAN engine whose input size is 224 x 224'):
        eng.strise_score(small, torch.zeros((200, 180, 3), dtype=torch.float64), cells[:, :1] % 17, shifts, (17, 15), SCALE, emb, emb, enc,
                         probe_shape=(200, 180), quantize=True)
    # a luminance engine without tables
    with pytest.raises(ValueError, match='needs the resampling tables'):
        lum(tables=None)
    # table entries
    with pytest.raises(ValueError, match=r'row table entry 5 has count 0, outside \[1, 8\]'):
        lum(tables=changed(0, 5, count=0))
    with pytest.raises(ValueError, match=r'column table entry 7 has count 9, outside \[1, 8\]'):
        lum(tables=changed(1, 7, count=9))
    with pytest.raises(ValueError, match='row table entry 127 reads .* a window outside the probe\'s 224'):
        lum(tables=changed(0, 127, first=222))
    with pytest.raises(ValueError, match='column table entry 0 reads .* a window outside'):
        lum(tables=changed(1, 0, first=-1))
    neg = tables[1]['coef'][3].copy()
    neg[1] = -4
    with pytest.raises(ValueError, match='column table entry 3 has the negative coefficient -4'):
        lum(tables=changed(1, 3, coef=neg))
    with pytest.raises(ValueError, match='more than 8 taps'):
        first, count, coef = BB.pil_bilinear_axis(224, 32)
        lum(tables=(dict(first=first, count=count, coef=coef),) * 2)
    # what check_masks refuses, against probe_h x probe_w
    with pytest.raises(ValueError, match='mask_scale 129 exceeds the 128 x 300 input'):
        eng.strise_masks(cells, shifts, (1, 3), 129, probe_shape=(128, 300), exact=True)
    with pytest.raises(ValueError, match='cell index 360 of mask 1 outside the 10 x 10 grid'):
        eng.strise_quantized(torch.zeros((120, 120, 3), dtype=torch.uint8), torch.zeros((120, 120, 3), dtype=torch.float64),
                             np.array([[5], [360]], dtype=np.int32), shifts[:2], (10, 10), SCALE, probe_shape=(120, 120))
    with pytest.raises(ValueError, match=r'masks \[-2, -2 \+ 1\) of 48'):
        eng.strise_quantized(probe, fill, cells, shifts, (19, 19), SCALE, first=-2, count=1)
    # the calls as they were refuse what they refused: Light-CNN on the named path
    with pytest.raises(ValueError, match='3-channel network'):
        e1.strise_score(torch.zeros((128, 128, 3), dtype=torch.uint8), torch.zeros((128, 128, 3), dtype=torch.float64), cells % 121, shifts, (11, 11), SCALE,
                        emb1, emb1, enc1)
    torch.cuda.synchronize()
    assert np.isfinite(lum()[0].cpu().numpy()).all()
