"""GPU tests of weighted subtree EBP as one engine call (xfr_weighted_subtree_ebp; Whitebox.weighted_subtree_ebp(..., native=True)): against
the real reference's goldens, against the Python selection loop on the same engine, batch against single probes, the visiting-order rule
and its callback, the uint8 versions of the generator, the failure modes and the C host."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import golden_cases as GC
from parity_utils import assert_map_close_robust, make_backbone, make_images
from xfr_amd import _lib, synth
from xfr_amd import inpainting_game as IG
from xfr_amd.models import whitebox as WB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mini(mode):
    bb, sd = make_backbone('stresnet_mini', seed=3, recipe='mild', num_classes=5)
    subj = GC.engine_subject('stresnet_mini', bb, mode)
    subj.wb.debug_trace = False
    subj.set_cls(synth.unit_rows(1, 512, seed=1) / 2500, synth.unit_rows(1, 512, seed=2) / 2500)
    return subj, make_images('stresnet_mini', 1, seed=5)


def _three(x0):
    n = 3
    x = torch.cat((x0, make_images('stresnet_mini', n - 1, seed=11)), dim=0)
    xm = torch.cat((synth.unit_rows(1, 512, seed=1), synth.unit_rows(n - 1, 512, seed=31)), dim=0) / 2500
    xn = torch.cat((synth.unit_rows(1, 512, seed=2), synth.unit_rows(n - 1, 512, seed=32)), dim=0) / 2500
    return x, xm, xn


def _check_golden(g, key, smap, P_valid, w_valid, k_valid):
    assert [int(k) for k in k_valid] == [int(k) for k in g[key + '/k_valid']]
    assert np.allclose(np.array(w_valid), g[key + '/w_valid'], rtol=1e-4, atol=0)
    for a, b in zip(P_valid, g[key + '/P_valid']):
        assert_map_close_robust(a, b, key + ' subtree map (native)')
    assert_map_close_robust(smap, g[key + '/map'], key + ' (native)')
    assert abs(float(np.sum(smap)) - 1.0) < 1e-4


@pytest.mark.parametrize('mode', ['norelu', 'affineonly_with_prior', 'all'])
def test_native_mini_golden(gpu_device, mode):
    g = GC.golden('golden_subtree_mini')
    subj, x = _mini(mode)
    res = subj.wb.weighted_subtree_ebp(x, 0, 1, topk=8, verbose=False, subtree_mode=mode, native=True)
    _check_golden(g, 'mini/%s/top8' % mode, *res)


def test_native_mini_golden_max_variant(gpu_device):
    g = GC.golden('golden_subtree_mini')
    subj, x = _mini('norelu')
    key = 'mini/norelu/top3max'
    smap, P_valid, w_valid, k_valid = subj.wb.weighted_subtree_ebp(x, 0, 1, topk=3, verbose=False, subtree_mode='norelu', do_max_subtree=True,
                                                                  native=True)
    assert [int(k) for k in k_valid] == [int(k) for k in g[key + '/k_valid']]
    assert np.allclose(np.array(w_valid), g[key + '/w_valid'], rtol=1e-4, atol=0)
    assert_map_close_robust(smap, g[key + '/map'], key + ' (native)')
    assert abs(float(np.sum(smap)) - 1.0) < 1e-4


def test_native_resnet101_golden(gpu_device):
    g = GC.golden('golden_subtree_r101')
    gold = GC.golden('golden_r101')
    bb, sd = make_backbone('stresnet101', seed=0, num_classes=65359)
    subj = GC.engine_subject('stresnet101', bb, 'norelu')
    subj.wb.debug_trace = False
    x_demo, x_probe, x_non, x_mate = GC.net_inputs('stresnet101')
    subj.set_cls((1.0 / 2500.0) * torch.from_numpy(gold['r101/norelu/enc_mate']), (1.0 / 2500.0) * torch.from_numpy(gold['r101/norelu/enc_nonmate']))
    key = 'r101/norelu/top32'
    smap, P_valid, w_valid, k_valid = subj.wb.weighted_subtree_ebp(x_probe, 0, 1, topk=32, verbose=False, subtree_mode='norelu', native=True)
    ref_k = [int(k) for k in g[key + '/k_valid']]
    # as test_gpu_subtree.py: layers whose weight ties with the weight at the cut may be chosen differently among themselves
    wk = dict(zip(ref_k, [float(v) for v in g[key + '/w_valid']]))
    wk.update(dict(zip([int(k) for k in k_valid], [float(v) for v in w_valid])))
    cut = min(wk[k] for k in ref_k)
    for k in set(k_valid) ^ set(ref_k):
        assert abs(wk[k] - cut) <= 1e-4 * cut, 'layer %d (weight %.6g) differs from the reference selection away from the cut (%.6g)' % (k, wk[k], cut)
    assert len(k_valid) == len(ref_k) == 32
    assert np.allclose(sorted(w_valid), sorted(g[key + '/w_valid']), rtol=1e-4)
    assert_map_close_robust(smap, g[key + '/map'], key + ' (native)', rtol=5e-3)
    assert abs(float(np.sum(smap)) - 1.0) < 1e-4


@pytest.mark.parametrize('gating', [True, False])
def test_native_equals_python_path(gpu_device, gating):
    """Same engine, same sweeps: the same selection, bit-identical top-k maps (pooled and blurred), and merged maps that differ only by the
    summation order of the merge."""
    subj, x0 = _mini('norelu')
    wb = subj.wb
    x, xm, xn = _three(x0)
    for sweep_batch in (None, 5):              # 5: several rounds, idle rows once a probe is done
        for sal in (True, False):
            kw = dict(topk=8, subtree_mode='norelu', do_mated_similarity_gating=gating, sweep_batch=sweep_batch, do_mwp_to_saliency=sal)
            py = wb.weighted_subtree_ebp_batch(x, xm, xn, **kw)
            nat = wb.weighted_subtree_ebp_batch(x, xm, xn, native=True, **kw)
            assert len(py) == len(nat) == 3
            for i, (a, b) in enumerate(zip(py, nat)):
                what = 'probe %d sweep_batch %s saliency %s' % (i, sweep_batch, sal)
                assert b[3] == a[3] and all(type(k) is int for k in b[3]), what
                assert b[2] == a[2] and all(type(w) is float for w in b[2]), what
                assert len(b[1]) == len(a[1]) and all(np.array_equal(p, q) for p, q in zip(a[1], b[1])), what
                sa, sb = np.asarray(a[0]), np.asarray(b[0])
                assert sb.dtype == sa.dtype == np.float32 and sb.shape == sa.shape
                assert np.abs(sb - sa).max() <= 1e-6 * np.abs(sa).max(), (what, np.abs(sb - sa).max() / np.abs(sa).max())
                if sal:
                    assert abs(float(sb.sum()) - 1.0) < 1e-4


@pytest.mark.parametrize('gating', [True, False])
def test_native_batch_equals_native_single(gpu_device, gating):
    subj, x0 = _mini('norelu')
    wb = subj.wb
    x, xm, xn = _three(x0)
    single = []
    for i in range(3):
        subj.set_cls(xm[i:i + 1], xn[i:i + 1])
        single.append(wb.weighted_subtree_ebp(x[i:i + 1], 0, 1, topk=8, verbose=False, subtree_mode='norelu', do_mated_similarity_gating=gating,
                                              native=True))
    for sweep_batch in (None, 5):
        batch = wb.weighted_subtree_ebp_batch(x, xm, xn, topk=8, subtree_mode='norelu', do_mated_similarity_gating=gating, sweep_batch=sweep_batch,
                                              native=True)
        for i in range(3):
            sm_b, P_b, w_b, k_b = batch[i]
            sm_s, P_s, w_s, k_s = single[i]
            assert sorted(k_b) == sorted(k_s), (i, k_b, k_s)
            assert np.allclose(sorted(w_b), sorted(w_s), rtol=1e-4)
            assert_map_close_robust(sm_b, sm_s, 'probe %d native batch vs native single' % i)


def _seeds(wb, xm, xn, eng):
    st = wb.net._program.marks['encode']
    return st, torch.stack((xm, xn, xm), dim=0).to(eng.device)


def test_order_rule_and_callback(gpu_device):
    subj, x0 = _mini('norelu')
    wb = subj.wb
    x, xm, xn = _three(x0)
    eng = wb._engine(3)
    st, seeds = _seeds(wb, xm, xn, eng)
    xd = x.to(eng.device)
    # the engine's rule is NumPy's stable argsort
    a = eng.weighted_subtree(xd, st, seeds, 8, order='engine')
    b = eng.weighted_subtree(xd, st, seeds, 8, order=lambda w, p: np.argsort(w.astype(np.float64), kind='stable'))
    assert all(np.array_equal(u.cpu().numpy() if torch.is_tensor(u) else u, v.cpu().numpy() if torch.is_tensor(v) else v) for u, v in zip(a, b))
    # the callback: once per probe, with the w column xfr_subtree_weights returns; the order it gives is the order used
    eng.hold_forward(True)                     # as the call itself and the Python path compute them: under one held forward
    try:
        w_ref, _ = eng.subtree_weights(xd, st, seeds[:2])
    finally:
        eng.hold_forward(False)
    calls = []

    def rec(w, probe):
        calls.append((probe, w.copy()))
        return np.argsort(w.astype(np.float64))
    smap, top, w_valid, k_valid, n_valid = eng.weighted_subtree(xd, st, seeds, 8, order=rec)
    assert [p for p, _ in calls] == [0, 1, 2]
    for p, w in calls:
        assert w.dtype == np.float32 and np.array_equal(w, w_ref[:, p])
    py = wb.weighted_subtree_ebp_batch(x, xm, xn, topk=8, subtree_mode='norelu')
    for i in range(3):
        assert [int(k) for k in k_valid[i, :n_valid[i]]] == py[i][3]
    # a callback that fails, or returns no permutation, fails the call
    with pytest.raises(ValueError, match='order_fn'):
        eng.weighted_subtree(xd, st, seeds, 8, order=lambda w, p: np.zeros(len(w), dtype=np.int64))


class _NativeWB(object):
    def __init__(self, wb):
        self._wb = wb

    def __getattr__(self, name):
        return getattr(self._wb, name)

    def weighted_subtree_ebp(self, *a, **k):
        return self._wb.weighted_subtree_ebp(*a, native=True, **k)


@pytest.mark.parametrize('key,ver,mode_w', [('c2/mini/v08_all_top8', 8, 'all'), ('c2/mini/v09_norelu_top8', 9, 'norelu'),
                                            ('c2/mini/v10_norelu_top8', 10, 'norelu')])
def test_native_uint8_versions(gpu_device, key, ver, mode_w):
    gold = GC.golden('golden_c2')
    bb, sd = make_backbone('stresnet_mini', seed=3, recipe='mild', num_classes=5)
    bb.to(gpu_device)
    wb = WB.Whitebox(WB.WhiteboxSTResnet(bb), ebp_version=ver, ebp_subtree_mode='norelu')
    wb._test_device = gpu_device
    im_mates, im_nonmates, probe = GC.c2_images()
    smap = IG.run_weighted_subtree_triplet_ebp(_NativeWB(wb), im_mates, im_nonmates, probe, 'resnetv4_pytorch', mode_w, ver, gpu_device, topk=8)
    want = gold[key + '/map']
    assert smap.dtype == np.uint8 and smap.shape == want.shape
    d = np.abs(smap.astype(int) - want.astype(int))
    assert d.max() <= 2 and (d > 0).mean() <= 0.02, '%s: max level diff %d, %.2f %% pixels differ' % (key, d.max(), 100 * (d > 0).mean())


def _raw(eng, x, st, seeds, topk, sweep_batch=0):
    n = x.shape[0]
    c1, h1, w1 = eng.tensor_shape(1)
    smap = torch.empty((n, h1, w1), device=eng.device)
    k = max(topk, 1)
    wv, kv, nv = np.zeros(n * k, np.float32), np.zeros(n * k, np.int32), np.zeros(n, np.int32)
    args = _lib.SubtreeArgs(topk, 1, 0, _lib.SUBTREE_SALIENCY, sweep_batch, _lib.SUBTREE_ORDER_FN(), None)
    st_ = eng.lib.xfr_weighted_subtree_ebp(eng._h, x.data_ptr(), n, int(st), seeds.data_ptr(), ctypes.byref(args), smap.data_ptr(), None,
                                           wv.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), kv.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                           nv.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream))
    torch.cuda.synchronize(eng.device)
    return st_, eng.lib.xfr_last_error().decode()


def test_failure_modes_release_the_held_forward(gpu_device):
    subj, x0 = _mini('norelu')
    wb = subj.wb
    x, xm, xn = _three(x0)
    eng = wb._engine(4)
    st, seeds = _seeds(wb, xm, xn, eng)
    xd = x.to(eng.device).contiguous()
    x4 = torch.cat((xd, xd[:1] * 0.5), dim=0).contiguous()
    ebp_seed = torch.stack((torch.cat((xm, xm[:1])), torch.cat((xn, xn[:1]))), dim=0).to(eng.device)

    def plain_ebp():
        lean0 = eng.lean_launches()
        _, pooled = eng.ebp(x4, st, ebp_seed)
        return pooled.cpu().numpy(), eng.lean_launches() - lean0
    before, lean_before = plain_ebp()
    # zero seeds: every prior is zero, no valid subtree -- the reference's RuntimeError, a failing status
    zeros = torch.zeros_like(seeds)
    with pytest.raises(RuntimeError, match='Failed to calculate valid subtrees. The ebp subtree mode \\(norelu\\) may not support'):
        eng.weighted_subtree(xd, st, zeros, 8)
    status, msg = _raw(eng, xd, st, zeros, 8)
    assert status != _lib.XFR_OK and 'Failed to calculate valid subtrees' in msg
    with pytest.raises(RuntimeError, match='Failed to calculate valid subtrees'):
        wb.weighted_subtree_ebp_batch(x, xm * 0, xn * 0, topk=8, subtree_mode='norelu', native=True)
    # topk 0 and more rows than the engine has
    status, msg = _raw(eng, xd, st, seeds, 0)
    assert status == _lib.XFR_INVALID_ARG and 'topk' in msg
    status, msg = _raw(eng, xd, st, seeds, 8, sweep_batch=2 * eng.max_batch // 3 + 1)
    assert status == _lib.XFR_INVALID_ARG and 'gradient rows' in msg
    after, lean_after = plain_ebp()
    assert np.array_equal(before, after) and lean_after == lean_before
    # ... and a good call still works on the same engine
    smap, top, w_valid, k_valid, n_valid = eng.weighted_subtree(xd, st, seeds, 8)
    assert (n_valid > 0).all() and np.isfinite(smap.cpu().numpy()).all()


def test_c_subtree_host_against_the_reference(tmp_path):
    csrc = os.path.join(ROOT, 'xfr_amd', 'csrc')
    exe = str(tmp_path / 'c_subtree')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'examples', 'c_subtree.c'),
                           '-L' + csrc, '-lxfr_amd', '-Wl,-rpath,' + csrc, '-ldl', '-lm', '-o', exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    g = GC.golden('golden_csubtree')
    m = re.search(r'(\d+) valid subtrees, firings((?: \d+ \(w [0-9.e+-]+\))+)', out.stdout)
    assert m and 1 <= int(m.group(1)) <= len(g['k_valid']), out.stdout
    # the engine's layerwise sweep gives firing 0 of this network an all-zero map (examples/c_subtree.c, "Known gap"): what it selects is a
    # subset of the reference's selection, in the same ascending-weight order
    got = [int(v) for v in re.findall(r' (\d+) \(w', m.group(2))]
    ref = [int(k) for k in g['k_valid']]
    assert set(got) <= set(ref) and got == [k for k in ref if k in got], (got, ref)
    assert 'firings among the reference\'s yes' in out.stdout, out.stdout
    r = re.search(r'map max\|d\|/max ([0-9.e+-]+), cosine ([0-9.]+)', out.stdout)
    assert r and float(r.group(1)) <= 1e-3 and float(r.group(2)) >= 0.99999, out.stdout
