"""The uint8 saliency tail on the device (xfr_amd/csrc/u8_tail.hip: xfr_mwp_to_saliency_u8, xfr_contrastive_u8, xfr_triplet_contrastive_u8tail,
XFR_SUBTREE_UINT8_SALIENCY) held to tests/u8_tail_inputs.truth TO THE BYTE, and its wiring through Engine, the drop-in Whitebox and the batched API.
The chain is integer arithmetic after one stretch whose operations are stated one by one, and tests/test_u8_tail_inputs.py proves the truth equal
to NumPy's and Pillow's own on every case without a device, so no case here carries an allowance.

Value-only mutations of u8_tail.hip, each built into a library of its own and run once on the MI355X against the 20 cases of this file, with what
caught each:
  (a) a box pass without its rounding term (1 << 23)            14 fail: test_tail_equals_the_truth at every shape but 1 x 1 (a single pixel is a
                                                                constant map: zeros either way), test_identity_levels_at_eps_1e12, both
                                                                test_contrastive_u8_is_raw_then_tail cases and the subtree case (their last
                                                                check holds the device tail to the truth), test_dropin_version_5_runs_no_pillow
  (b) zero padding instead of the replicated edge               the same 14
  (c) the uint8 stretch as the integer floor(255 (v - mn) / d)  10 fail: test_tail_equals_the_truth at every shape but 1 x 1 (eps = 1e-12, where
                                                                the float64 form sits one level lower) and test_identity_levels_at_eps_1e12;
                                                                the engine-side cases run at eps = 1e-16, where the two forms agree
The six cases that pass under (a) and (b) compare two runs of the same kernels (wiring) or call nothing (refusals).
"""
import ctypes

import numpy as np
import PIL.Image
import pytest
import torch

import golden_cases as GC
import layer_nets as L
import u8_tail_inputs as U
from parity_utils import make_backbone, make_images
from xfr_amd import _lib, synth
from xfr_amd import inpainting_game as IG
from xfr_amd.engine import Engine
from xfr_amd.models import whitebox as WB

pytestmark = pytest.mark.gpu

MFM128 = L.NetCase('mfm128', (1, 128, 128), L._mfm((64, 64)), "the Light-CNN catalogue net at Light-CNN's own size: 128 x 128 maps", 7)
_ENGINES = {}
_MINI = {}


@pytest.fixture(scope='module', autouse=True)
def _engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()
    _MINI.clear()


def _engine(name, device):
    if name not in _ENGINES:
        case = MFM128 if name == 'mfm128' else L.BY_NAME[name]
        e = Engine(case.program(), 8, device)
        e.load_weights(case.params())
        _ENGINES[name] = e
    return _ENGINES[name]


def _mini(device, ver):
    """A drop-in Whitebox of the mini STR-ResNet at ebp_version `ver`, with three probes and their classifier rows."""
    if ver not in _MINI:
        bb, sd = make_backbone('stresnet_mini', seed=3, recipe='mild', num_classes=5)
        bb.to(device)
        wb = WB.Whitebox(WB.WhiteboxSTResnet(bb), ebp_version=ver, ebp_subtree_mode='norelu')
        x = make_images('stresnet_mini', 3, seed=5)
        xm = torch.cat((synth.unit_rows(1, 512, seed=1), synth.unit_rows(2, 512, seed=31)), dim=0) / 2500
        xn = torch.cat((synth.unit_rows(1, 512, seed=2), synth.unit_rows(2, 512, seed=32)), dim=0) / 2500
        _MINI[ver] = (wb, x, xm, xn)
    return _MINI[ver]


def _host_chain(wb, maps):
    """Whitebox._mwp_to_saliency's host branch, map by map: what the device tail replaces."""
    assert wb.convert_saliency_uint8
    return np.stack([wb._mwp_to_saliency(np.array(m)) for m in maps])


def _same(tag, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, want.dtype, got.shape, want.shape)
    wrong = got != want
    print('%s: %d of %d values differ' % (tag, int(wrong.sum()), wrong.size))
    assert not wrong.any(), '%s: %d of %d differ, first at %s: %r, want %r' % (tag, int(wrong.sum()), wrong.size, tuple(np.argwhere(wrong)[0]),
                                                                               got[wrong][0], want[wrong][0])


@pytest.mark.parametrize('shape', U.SHAPES, ids=['%dx%d' % s for s in U.SHAPES])
def test_tail_equals_the_truth(gpu_device, shape):
    """Both forms of stage A, both eps, every family; 1, 3 and 2 * max_batch + 1 maps in one call (the wrapper's second and third chunk)."""
    eng = _engine('stem', gpu_device)
    for eps in U.EPS:
        eng.set_mode('affineonly_with_prior', eps)
        for fams in (U.F32_FAMILIES, U.U8_FAMILIES):
            for n in (1, 3, 2 * eng.max_batch + 1):
                pick = [fams[(i + n) % len(fams)] for i in range(n)]          # n = 17 takes every family, 1 and 3 start elsewhere
                maps = np.stack([U.case(f, shape) for f in pick])
                want = np.stack([U.case_truth(f, shape, eps) for f in pick])
                got = eng.mwp_to_saliency_u8(torch.as_tensor(maps.copy())).cpu().numpy()
                _same('%s eps %g %s n %d' % (shape, eps, maps.dtype, n), got, want)
    assert 2 * eng.max_batch + 1 >= len(U.F32_FAMILIES)


def test_identity_levels_at_eps_1e12(gpu_device):
    """The literal float64 form of the uint8 stretch: the identity 0..255 at eps = 1e-12 starts one level lower."""
    eng = _engine('stem', gpu_device)
    eng.set_mode('affineonly_with_prior', 1e-12)
    got = eng.mwp_to_saliency_u8(torch.as_tensor(U.IDENTITY.copy())[None]).cpu().numpy()[0]
    _same('identity', got, U.truth(U.IDENTITY, 1e-12))
    assert not np.array_equal(U.truth(U.IDENTITY, 1e-12), U.truth(U.IDENTITY, 1e-16))


def test_refusals(gpu_device):
    eng = _engine('stem', gpu_device)
    f = torch.zeros((1, 4, 4), device=gpu_device)
    b = torch.zeros((1, 4, 4), device=gpu_device, dtype=torch.uint8)
    out = torch.full((1, 4, 4), 7, device=gpu_device, dtype=torch.uint8)
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)

    def refused(pattern, pf=f.data_ptr(), pb=None, n=1, h=4, w=4, o=out.data_ptr()):
        with torch.cuda.device(gpu_device):
            status = eng.lib.xfr_mwp_to_saliency_u8(eng._h, pf, pb, n, h, w, o, stream)
        assert status == _lib.XFR_INVALID_ARG, (pattern, status)
        with pytest.raises(ValueError, match=pattern):
            _lib.check(status)

    refused('exactly one of pooled_dev and levels_dev must be given, got both', pb=b.data_ptr())
    refused('exactly one of pooled_dev and levels_dev must be given, got neither', pf=None)
    refused(r'h 257, w 256', h=257, w=256)
    refused(r'h 1, w 65537', h=1, w=65537)
    refused(r'n 0', n=0)
    refused(r'h 0', h=0)
    refused('null argument', o=None)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7).all()
    with pytest.raises(ValueError, match='tail must be'):
        eng.contrastive(torch.zeros((1, 3, 37, 29)), 2, torch.zeros((2, 1, 5)), None, raw=True, tail='u8')


def _net(name, device):
    """-> (engine, seed tensor, inputs(n), seeds(n)) of 'stresnet_mini' or the Light-CNN catalogue net at 128 x 128."""
    if name == 'mfm128':
        eng = _engine('mfm128', device)
        eng.set_mode('affineonly_with_prior', 1e-16)
        st = MFM128.program().marks['classify']
        d = int(np.prod(eng.tensor_shape(st)))
        return (eng, st, lambda n: MFM128.inputs(n, seed=3).to(device),
                lambda n: torch.rand((2, n, d), generator=torch.Generator().manual_seed(222)).to(device))
    wb, x, xm, xn = _mini(device, 5)
    eng = wb._engine(3)
    return eng, wb.net._program.marks['encode'], lambda n: x[:n].to(device), lambda n: torch.stack((xm[:n], xn[:n]), dim=0).to(device)


@pytest.mark.parametrize('name', ['stresnet_mini', 'mfm128'])
def test_contrastive_u8_is_raw_then_tail(gpu_device, name):
    eng, st, inputs, seeds = _net(name, gpu_device)
    h1, w1 = eng.tensor_shape(1)[1:]
    assert (h1, w1) == ((128, 128) if name == 'mfm128' else (112, 112))
    for n in (1, 3):
        x, s = inputs(n), seeds(n)
        for pct in (None, 20.0):
            raw = eng.contrastive(x, st, s, pct, raw=True)
            raw2 = eng.contrastive(x, st, s, pct, raw=True)
            _same('%s n %d pct %s: two raw calls' % (name, n, pct), raw.cpu().numpy().view(np.uint32), raw2.cpu().numpy().view(np.uint32))
            assert float(raw.max()) > 0
            want = eng.mwp_to_saliency_u8(raw).cpu().numpy()
            got = eng.contrastive(x, st, s, pct, tail='u8')
            assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h1, w1)
            _same('%s n %d pct %s: xfr_contrastive_u8' % (name, n, pct), got.cpu().numpy(), want)
            _same('%s n %d pct %s: tail of raw against the truth' % (name, n, pct), want,
                  np.stack([U.truth(m, 1e-16) for m in raw.cpu().numpy()]))
            assert want.max() == 255


@pytest.mark.parametrize('name', ['stresnet_mini', 'mfm128'])
def test_triplet_u8tail_is_raw_then_tail(gpu_device, name):
    """The fused triplet step: its float (version 6) form first equals xfr_contrastive seeded with scale * encode(gallery), bit for bit, so that the
    raw counterpart of the uint8 form is xfr_contrastive_raw with those seeds."""
    eng, st, inputs, _ = _net(name, gpu_device)
    scale = 1.0 / 2500.0
    for n in (1, 3):
        x = inputs(n)
        gallery = torch.cat((inputs(3)[:n] * 0.5, inputs(3)[3 - n:] * 0.25 + 1.0), dim=0).contiguous()
        enc = eng.forward(gallery, st).reshape(2, n, -1)
        s = enc * torch.tensor(scale, dtype=torch.float32, device=enc.device)
        for pct in (None, 20.0):
            a = eng.triplet_contrastive(x, gallery, st, scale, pct).cpu().numpy()
            b = eng.contrastive(x, st, s, pct).cpu().numpy()
            _same('%s n %d pct %s: triplet step against contrastive, version 6' % (name, n, pct), a.view(np.uint32), b.view(np.uint32))
            want = eng.mwp_to_saliency_u8(eng.contrastive(x, st, s, pct, raw=True)).cpu().numpy()
            got = eng.triplet_contrastive(x, gallery, st, scale, pct, tail='u8')
            assert got.dtype == torch.uint8
            _same('%s n %d pct %s: xfr_triplet_contrastive_u8tail' % (name, n, pct), got.cpu().numpy(), want)


def test_subtree_uint8_saliency_is_uint8_then_tail(gpu_device):
    wb, x, xm, xn = _mini(gpu_device, 5)
    eng = wb._engine(3)
    eng.set_mode('norelu', wb.eps, False)
    st = wb.net._program.marks['encode']
    n, topk = 2, 4
    xd = x[:n].to(gpu_device)
    seeds = torch.stack((xm[:n], xn[:n], xm[:n]), dim=0).to(gpu_device)
    smap, top, w_valid, k_valid, n_valid = eng.weighted_subtree(xd, st, seeds, topk, output='uint8')
    smap2, top2, w2, k2, n2 = eng.weighted_subtree(xd, st, seeds, topk, output='uint8_saliency')
    assert np.array_equal(k_valid, k2) and np.array_equal(n_valid, n2) and np.array_equal(w_valid, w2) and (n_valid > 0).all()
    levels = smap.cpu().numpy()
    assert np.array_equal(levels, np.round(levels)) and levels.min() == 0 and levels.max() <= 255
    want = eng.mwp_to_saliency_u8(smap.to(torch.uint8)).cpu().numpy()
    _same('merged map', smap2.cpu().numpy(), want.astype(np.float32))
    h1, w1 = top.shape[-2:]
    want_top = eng.mwp_to_saliency_u8(top.reshape(n * topk, h1, w1)).cpu().numpy().reshape(n, topk, h1, w1)
    _same('top-k maps', top2.cpu().numpy(), want_top.astype(np.float32))
    for b in range(n):
        assert want_top[b, :n_valid[b]].reshape(n_valid[b], -1).max(axis=1).min() == 255 and not want_top[b, n_valid[b]:].any()
    _same('merged map against the truth', want, np.stack([U.truth(m.astype(np.uint8), wb.eps) for m in levels]))


def test_dropin_version_5_runs_no_pillow(gpu_device, monkeypatch):
    """Whitebox(ebp_version=5): contrastive_ebp, truncated_contrastive_ebp and the native weighted subtree return exactly what the host chain makes
    of the raw maps, without a call of Pillow's filter."""
    wb, x, xm, xn = _mini(gpu_device, 5)
    eng = wb._engine(3)
    st = wb.net._program.marks['encode']
    pil_filter = PIL.Image.Image.filter

    def no_pillow(self, *a, **k):
        raise AssertionError('PIL.Image.Image.filter called')
    wb.net.set_triplet_classifier(xm[0:1], xn[0:1])
    for n in (1, 3):
        xd = x[:n].to(gpu_device)
        for pct in (None, 20):
            eng = wb._engine(n)
            st, seeds = wb._class_seeds(n, 0, 1)         # the seeds the drop-in methods sweep with: the one installed classifier for every image
            raw = eng.contrastive(xd, st, seeds, None if pct is None else float(pct), raw=True).cpu().numpy()
            want = _host_chain(wb, raw)
            monkeypatch.setattr(PIL.Image.Image, 'filter', no_pillow)
            try:
                got = wb.contrastive_ebp(xd, 0, 1) if pct is None else wb.truncated_contrastive_ebp(xd, 0, 1, percentile=pct)
            finally:
                monkeypatch.setattr(PIL.Image.Image, 'filter', pil_filter)
            _same('drop-in n %d pct %s' % (n, pct), got, want[0] if n == 1 else want)
    # the native weighted subtree, merged map and top-k maps
    wb.net.set_triplet_classifier(xm[0:1] * 2500, xn[0:1] * 2500)
    eng.set_mode('norelu', wb.eps, False)
    seeds = torch.stack((xm[0:1] * 2500, xn[0:1] * 2500, xm[0:1] * 2500), dim=0).to(gpu_device)
    smap, top, w_valid, k_valid, n_valid = eng.weighted_subtree(x[:1].to(gpu_device), st, seeds, 4, output='uint8')
    want_map = _host_chain(wb, smap.cpu().numpy().astype(np.uint8))[0]
    want_top = _host_chain(wb, top.cpu().numpy()[0, :n_valid[0]])
    monkeypatch.setattr(PIL.Image.Image, 'filter', no_pillow)
    try:
        got = wb.weighted_subtree_ebp(x[:1].to(gpu_device), 0, 1, topk=4, verbose=False, subtree_mode='norelu', native=True)
    finally:
        monkeypatch.setattr(PIL.Image.Image, 'filter', pil_filter)
    assert got[3] == [int(k) for k in k_valid[0, :n_valid[0]]]
    _same('drop-in weighted subtree, merged', got[0], want_map)
    _same('drop-in weighted subtree, top-k', np.stack(got[1]), want_top)


def test_batch_api_default_is_v6(gpu_device):
    """`tail` left out is tail='v6', bit for bit, whatever the Whitebox's version; 'uint8' and 'version' give the bytes of the device tail."""
    wb, x, xm, xn = _mini(gpu_device, 5)
    xd = x.to(gpu_device)
    bits = lambda t: t.cpu().numpy().view(np.uint32)          # noqa: E731
    for pct in (None, 20):
        a = wb.contrastive_triplet_ebp_batch(xd, xm, xn, percentile=pct)
        b = wb.contrastive_triplet_ebp_batch(xd, xm, xn, percentile=pct, tail='v6')
        assert a.dtype == torch.float32
        _same('contrastive_triplet_ebp_batch pct %s' % pct, bits(a), bits(b))
        u = wb.contrastive_triplet_ebp_batch(xd, xm, xn, percentile=pct, tail='version')
        v = wb.contrastive_triplet_ebp_batch(xd, xm, xn, percentile=pct, tail='uint8')
        assert u.dtype == torch.uint8
        _same('tail version / uint8', u.cpu().numpy(), v.cpu().numpy())
    n = 2
    mates, nonmates = xd[:n] * 0.5, xd[1:1 + n] * 0.25 + 1.0
    a = wb.triplet_images_ebp_batch(xd[:n], mates, nonmates)
    b = wb.triplet_images_ebp_batch(xd[:n], mates, nonmates, tail='v6')
    _same('triplet_images_ebp_batch', bits(a), bits(b))
    assert wb.triplet_images_ebp_batch(xd[:n], mates, nonmates, tail='version').dtype == torch.uint8
    for native in (False, True):
        a = wb.weighted_subtree_ebp_batch(xd[:n], xm[:n] * 2500, xn[:n] * 2500, topk=4, native=native)
        b = wb.weighted_subtree_ebp_batch(xd[:n], xm[:n] * 2500, xn[:n] * 2500, topk=4, native=native, tail='v6')
        for p, q in zip(a, b):
            _same('weighted_subtree_ebp_batch native %s' % native, p[0], q[0])
            assert p[3] == q[3] and p[0].dtype == np.uint8
    with pytest.raises(ValueError, match='tail must be'):
        wb.contrastive_triplet_ebp_batch(xd, xm, xn, tail='v5')
    # a version-6 Whitebox: 'version' is 'v6'
    wb6 = WB.Whitebox(wb.net, ebp_version=6, ebp_subtree_mode='norelu')
    a = wb6.contrastive_triplet_ebp_batch(xd, xm, xn)
    b = wb6.contrastive_triplet_ebp_batch(xd, xm, xn, tail='version')
    assert b.dtype == torch.float32
    _same('version 6, tail version', bits(a), bits(b))


def test_run_jobs_batched_tail_version(gpu_device):
    """run_jobs_batched(tail='version') at ebp_version 7: uint8 maps, equal to the per-job drop-in calls of the same Whitebox under the classifier
    rows the group computes.  The engine runs its batch-invariant arithmetic here (no tail balancing, literal schedule, fp32 GEMMs), so that a
    probe's float map -- hence its bytes -- does not depend on whether it is swept alone or in the group (include/xfr_amd.h)."""
    ver, mode_w, topk = 7, 'norelu', 4
    bb, sd = make_backbone('stresnet_mini', seed=3, recipe='mild', num_classes=5)
    bb.to(gpu_device)
    wb = WB.Whitebox(WB.WhiteboxSTResnet(bb), ebp_version=ver, ebp_subtree_mode='norelu')
    eng = wb._engine(2)
    eng.set_tail_balance(False)
    eng.set_lean(False)
    eng.set_split_gemm(0)
    im_mates, im_nonmates, probe = GC.c2_images()
    jobs = [(im_mates, im_nonmates, probe), (im_nonmates[:2], im_mates, im_nonmates[2])]
    methods = ('contrastive', 'truncated', 'weighted-subtree')
    out = IG.run_jobs_batched(wb, jobs, 'resnetv4_pytorch', mode_w, ver, gpu_device, topk=topk, methods=methods, native_subtree=True, tail='version')
    v6 = IG.run_jobs_batched(wb, jobs, 'resnetv4_pytorch', mode_w, ver, gpu_device, topk=topk, methods=methods[:2], native_subtree=True)
    dflt = IG.run_jobs_batched(wb, jobs, 'resnetv4_pytorch', mode_w, ver, gpu_device, topk=topk, methods=methods[:2], native_subtree=True, tail='v6')
    for m in methods[:2]:
        for a, b in zip(v6[m], dflt[m]):
            assert a.dtype == np.float32
            _same('%s: default against v6' % m, a.view(np.uint32), b.view(np.uint32))
    # the classifier rows as run_jobs_batched forms them
    enc = IG.encode_images(wb, [im for j in jobs for im in list(j[0]) + list(j[1])], gpu_device, wb.batch_size, 'auto')
    xm, xn, o = [], [], 0
    for j in jobs:
        a, b = len(j[0]), len(j[1])
        m_, n_ = enc[o:o + a].mean(dim=0, keepdim=True), enc[o + a:o + a + b].mean(dim=0, keepdim=True)
        xm.append(m_ / torch.norm(m_))
        xn.append(n_ / torch.norm(n_))
        o += a + b
    do_max, gating = IG.SUBTREE_VERSIONS[ver]
    for i, j in enumerate(jobs):
        x = wb.convert_from_numpy(j[2]).to(gpu_device)
        wb.net.set_triplet_classifier(xm[i] / 2500.0, xn[i] / 2500.0)
        want = {'contrastive': wb.contrastive_ebp(x, 0, 1), 'truncated': wb.truncated_contrastive_ebp(x, 0, 1, percentile=20)}
        wb.net.set_triplet_classifier(xm[i], xn[i])
        want['weighted-subtree'] = wb.weighted_subtree_ebp(x, 0, 1, topk=topk, verbose=False, do_max_subtree=do_max, subtree_mode=mode_w,
                                                           do_mated_similarity_gating=gating, native=True)[0]
        for m in methods:
            assert out[m][i].dtype == np.uint8 and out[m][i].shape == (112, 112)
            _same('job %d %s' % (i, m), out[m][i], want[m])
