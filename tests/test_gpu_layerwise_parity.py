"""Float64 parity of the "next" rows (xfr_amd/csrc/subtree.hip) on the catalogue of small layer programs (tests/layer_nets.py): the layer weights and
argmax elements of xfr_subtree_weights, the captures of xfr_ebp_capture, the prior injection, prefix launches and on-demand zeroing of
xfr_layerwise_ebp, and the gather / reverse / merge tail of xfr_weighted_subtree_ebp -- at odd HW, with MaxFeatureMap, pool pairs, stride-3
scatters, global pools, the normalize tail and a signed map, none of which stresnet_mini (test_gpu_subtree.py) has.

The truths come from tests/layerwise_inputs.py (the oracle tape in float64, with the float32 tape as the yardstick of precision); the rule is the one of
tests/parity_harness.py, for every tensor:  e_eng = max|engine - fp64| / max|fp64| <= max(K_RATIO * e32, FLOOR) with K_RATIO 4 and FLOOR 2e-6, and a map
whose truth is identically zero must be identically zero.  XFR_LAYERWISE_PARITY_REPORT=<path> writes every measured (e_eng, e32, cond) there as JSON.

Layerwise rows are held to  e_eng <= max(K_RATIO * e32 + cond, FLOOR)  instead: with a one-element prior the map is a product of a few individual
activations (1 / x[elem] at the prior's hook, a / x at the elementwise hooks behind it), each carrying the relative error E / v of its float32 forward
pass, and the row's own e32 is one draw of that lottery; cond = sum E32(tensor) / v64 states the allowance from the float32 tape's absolute error on
those tensors (layerwise_inputs.one_element_cond).  Measured on the MI355X with the plain rule: 80 of 11519 layerwise rows and 9
of 470 dense ones outside it (e_eng / e32 up to 76, e_eng up to 9.3e-5), every one of them the truth times 1 + d with a remainder below 2e-7 and d the
relative error of the engine's activation at that element, the engine's absolute error on those tensors 1.0 .. 1.6 times the float32 tape's.  With cond
(factor 1) the rows that need it use at most 46 % of e32 + cond; cond itself is held small on the CPU (test_layerwise_inputs.test_allowances_stay_small).  The other parts keep the plain rule: weights e_eng <= 5.5e-7 (e32 2e-10 .. 4.0e-7),
captures e_eng <= 1.1e-6, subtree top maps and merged maps e_eng <= 1.4e-6, all under the floor; the tightest comparison of the file uses 72 % of its bound
(avg_shortcut_v4, top 8, P[10]).  All 1272 rows of the weight pass are clear with the inputs chosen, 88 of them exact ties.

Value-only mutations of the engine, each tried once on a scratch build (never committed), with the test of this file that caught it; the older subtree
tests (test_gpu_subtree.py, test_gpu_subtree_native.py, without the ResNet-101 golden and the tool tests) pass all but the last:
  subtree_stats_kernel, in-thread tie-break `(int)e < bi` as `>`      test_layer_weights_and_elements [global_4225] (idx 12804 where 12675 is due; the 20
                                                                      catalogue nets pass: none has tied maxima 4096 elements apart)
  prior_val[sb] x (1 + 2^-10) in the float4 interpreter (ew_interp.h)  test_layerwise_sweeps, first at [stem] P[1] (e_eng 9.8e-4)
  the same in the scalar kernel (ew_chain_kernel)                      test_layerwise_sweeps, first at [stem] P[6], the 19 x 15 tap (e_eng 9.8e-4)
  run_backward: rows = SBa for scalar chains                           test_layerwise_sweeps [bf16x6], [halo64], [valid_wide] (idle rows of the ascending calls hold up to
                                                                      5.5e-3) and test_zeroing_bookkeeping_on_every_net (the default digest of those three nets differs
                                                                      from the poisoned and the eager one; the poisoned child stays finite: fmaxf(g, 0) swallows the NaN)
  gather_rows_kernel's scalar path copying HW - 1 elements             test_weighted_subtree_tail [stem] (a top map's last pixel 0 where 2.5e-4 is due)
  subtree_merge_kernel: t[0].wn for every slot                         test_weighted_subtree_tail [stem] (merged map all zero); also 11 tests of
                                                                      test_gpu_subtree_native.py (the golden, Python-path, batch and uint8 comparisons)
The file also found a bug: xfr_subtree_weights on its own left the raw MaxFeatureMap rows unwritten where the fused forward applies ([mfm_pool2]: w of
firing 5 0.0865 for every image, float64 0.259 / 0.222 / 0.267); fixed in forward.hip / subtree.hip (forward_all's keep_raw).  And a second: in an
ascending call, the maps of a sweep that is idle for every image held what an earlier call had left in P[-2] (9 of the 20 nets, up to 0.37 where zero is
due); layerwise_run now zeroes those rows (subtree.hip).
"""
import hashlib
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import layer_nets as L
import layerwise_inputs as W
from parity_harness import FLOOR, K_RATIO, Harness
from xfr_amd.engine import Engine

pytestmark = pytest.mark.gpu

# one subtree mode per net for the parts that need only one (test_gpu_layer_parity.SCHEDULE_MODE, restated: all four across the catalogue)
NET_MODE = {'stem': 'affineonly_with_prior', 'projection': 'norelu', 'avg_shortcut': 'all', 'bf16x6': 'affineonly_with_prior',
            'halo64': 'affineonly', 'halo65': 'all', 'mfm': 'affineonly', 'classifier': 'norelu', 'valid_wide': 'affineonly_with_prior',
            'strided': 'all', 'stem_rows': 'norelu', 'ceil_rows': 'all', 'pool_generic': 'affineonly', 'pool_odd17': 'affineonly_with_prior',
            'mfm_pool2': 'norelu', 'avg_shortcut_v4': 'affineonly', 'encode_tail': 'all', 'global_big': 'affineonly_with_prior',
            'avg_generic': 'norelu', 'signed_tail': 'affineonly', 'global_4225': 'all'}
NAMES = [c.name for c in L.CASES]
F32, F64 = torch.float32, torch.float64
# without the variable a row at or under FLOOR is recorded without its e32, which costs a sweep of the float32 tape (Harness.rule)
h = Harness(report_all=bool(os.environ.get('XFR_LAYERWISE_PARITY_REPORT')))
_engine, _rule = h.engine, h.rule


@pytest.fixture(scope='module', autouse=True)
def _engines_and_report():
    yield
    h.finish('XFR_LAYERWISE_PARITY_REPORT', merge=False)


def _setup(name, device):
    case = W.BY_NAME[name]
    eng = _engine(case, device)
    st = case.program().marks['classify']
    return case, eng, st, eng.firing_count(st)


@pytest.mark.parametrize('name', NAMES + [W.TIE_CASE.name])
def test_layer_weights_and_elements(gpu_device, name):
    """Engine.subtree_weights, both gates, one and three images: w per sample over the vector of firings under the rule; idx equal to the float64 first
    argmax in EVERY clear row (layerwise_inputs.CLEAR_GAP; exact ties included: the first index wins), within 1e-4 x scale of the maximum in the
    others; firings that share a gradient tensor report identical (w, idx).  global_4225 (layerwise_inputs.TIE_CASE) has its tied maxima 4096 elements
    apart, where one thread of subtree_stats_kernel meets both."""
    case, eng, st, nf = _setup(name, gpu_device)
    eng.set_mode(NET_MODE[name])            # the pass uses the plain weights: any mode
    bad = []
    for n in (1, 3):
        x = W.images(case, n).to(gpu_device)
        seed = torch.stack(W.onehot_seeds(case, n), 0)
        for gate in (True, False):
            t64, t32 = W.weights(case, n, gate, F64), W.weights(case, n, gate, F32)
            w, idx = eng.subtree_weights(x, st, seed, gate)
            assert w.shape == idx.shape == (nf, n) == t64['w'].shape, (name, w.shape, t64['w'].shape)
            tag = '%s/n%d/%s' % (name, n, 'ge0' if gate else 'lt0')
            for b in range(n):
                _rule(bad, 'weights/%s/sample%d' % (tag, b), w[:, b], t32['w'][:, b], t64['w'][:, b])
            for k in range(nf):
                for b in range(n):
                    v = t64['v'][k][b]
                    i = int(idx[k, b])
                    if not 0 <= i < v.numel():
                        bad.append('%s: firing %d sample %d: idx %d outside [0, %d)' % (tag, k, b, i, v.numel()))
                    elif t64['clear'][k, b]:
                        if i != int(t64['idx'][k, b]):
                            bad.append('%s: firing %d sample %d (clear, gap %.2e): idx %d, fp64 %d' % (tag, k, b, t64['gap'][k, b], i, int(t64['idx'][k, b])))
                    elif float(v[i]) < t64['w'][k, b] - 1e-4 * t64['scale'][k, b]:
                        bad.append('%s: firing %d sample %d: v64[idx %d] = %.9g, max %.9g' % (tag, k, b, i, float(v[i]), t64['w'][k, b]))
                if t64['shared'][k] and not (np.array_equal(w[k].view(np.uint32), w[k - 1].view(np.uint32)) and np.array_equal(idx[k], idx[k - 1])):
                    bad.append('%s: firings %d and %d share a gradient tensor and differ' % (tag, k - 1, k))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name', NAMES)
def test_captures(gpu_device, name):
    """Engine.ebp_capture at every firing, for the three elements of layerwise_inputs.prior_elements, four modes, three images in one call and then image 0
    of the three alone (same elements, same truth: the tape's samples are independent):
    |cap - P64[k][elem]| <= max(4 e32_k, FLOOR) max|P64[k]| with e32_k the float32 tape's error on P[k] (of the images in the call); elements of -1
    return 0."""
    case, eng, st, nf = _setup(name, gpu_device)
    bad = []
    for mode in W.MODES:
        eng.set_mode(mode)
        for n in (3, 1):
            x = W.images(case, 3)[:n].to(gpu_device)
            seed = W.ebp_seed(case, 3)[:n].unsqueeze(0)
            P32, P64 = [p[:n] for p in W.plain_P(case, 3, mode, F32)], [p[:n] for p in W.plain_P(case, 3, mode, F64)]
            elems = W.element_table(case, 3, mode)[0][:, :, :n]
            holes = elems[:, 0, :].copy()
            holes[(np.arange(nf) % 2) == 0] = -1
            for s, el in enumerate([elems[:, 0, :], elems[:, 1, :], elems[:, 2, :], holes]):
                cap = np.asarray(eng.ebp_capture(x, st, seed, el)).reshape(nf, n)
                for k in range(nf):
                    scale = float(P64[k].abs().max())
                    e32 = float((P32[k].double() - P64[k]).abs().max()) / max(scale, 1e-300)
                    flat = P64[k].flatten(1)
                    for b in range(n):
                        key = 'capture/%s/%s/n%d/P[%d]/slot%d/sample%d' % (name, mode, n, k, s, b)
                        if el[k, b] < 0:
                            if cap[k, b] != 0:
                                bad.append('%s: element -1 returned %.9g' % (key, cap[k, b]))
                            continue
                        want = float(flat[b, int(el[k, b])])
                        err = abs(float(cap[k, b]) - want) / scale
                        h.report[key] = (err, e32)
                        if not err <= max(K_RATIO * e32, FLOOR):
                            bad.append('%s: element %d: engine %.9g, fp64 %.9g, error / max|P| %.3e > max(4 x %.3e, %g)' % (
                                key, int(el[k, b]), cap[k, b], want, err, e32, FLOOR))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name', NAMES)
def test_layerwise_sweeps(gpu_device, name):
    """Engine.layerwise with element priors, four modes, three images, five sweeps per call until every (firing, element) pair has been a row, in three
    forms of the same rows (layerwise_inputs.layerwise_calls): ascending (prefix launches, on-demand zeroing), descending (whole launches), staggered
    (one image starting later), each call with a sweep that is idle for every image, chunk by chunk in the order descending, ascending, staggered (the
    idle rows of a prefix call then lie where the call before left live gradients).  Every row under the rule against layerwise_truth; idle rows and rows
    whose truth is zero are zero.
    One image: a dense prior, float32(P64[k]) times a seeded 0 / 1 mask, at every firing."""
    case, eng, st, nf = _setup(name, gpu_device)
    n = 3
    x = W.images(case, n).to(gpu_device)
    x1 = W.images(case, 1).to(gpu_device)
    bad = []
    for mode in W.MODES:
        eng.set_mode(mode)
        for form, c, (F, E, V, src) in W.interleaved_calls(case, n, mode):
            maps = eng.layerwise(x, st, F, E, V).cpu()
            assert tuple(maps.shape[:2]) == F.shape
            for j in range(F.shape[0]):
                for b in range(n):
                    key = 'layerwise/%s/%s/%s/call%d/row%d.%d' % (name, mode, form, c, j, b)
                    if src[j][b] is None:
                        if float(maps[j, b].abs().max()) != 0:
                            bad.append('%s: an idle row holds max|.| %.3e' % (key, float(maps[j, b].abs().max())))
                        continue
                    k, s = src[j][b]
                    m64, cond = W.layerwise_map_cond(case, n, mode, k, s, F64)
                    _rule(bad, key + '/P[%d]/slot%d' % (k, s), maps[j, b], lambda: W.layerwise_map(case, n, mode, k, s, F32)[b], m64[b], cond[b])
        for k in range(nf):
            prior, m64, cond = W.dense_truth(case, mode, k, F64)
            got = eng.layerwise(x1, st, [k], dense_prior=prior)
            _rule(bad, 'dense/%s/%s/P[%d]' % (name, mode, k), got.reshape(m64.shape), lambda: W.dense_truth(case, mode, k, F32)[1], m64, cond or 0.0)
    assert not bad, '\n'.join(bad)


def zeroing_child(path):
    """Child process of test_zeroing_bookkeeping_on_every_net: the interleaved calls of every net (read from `path`), one sha256 per net."""
    with open(path, 'rb') as f:
        jobs = pickle.load(f)
    dev = torch.device('cuda', 0)
    for name, mode, x, calls in jobs:
        case = L.BY_NAME[name]
        eng = Engine(case.program(), 8, dev)
        try:
            eng.load_weights(case.params())
            eng.set_mode(mode)
            st = case.program().marks['classify']
            h = hashlib.sha256()
            finite = True
            for (F, E, V) in calls:
                m = eng.layerwise(x.to(dev), st, F, E, V).cpu().numpy()
                finite = finite and bool(np.isfinite(m).all())
                h.update(np.ascontiguousarray(m, dtype=np.float32).tobytes())
            print('DIGEST %s %s %s' % (name, h.hexdigest(), 'finite' if finite else 'NONFINITE'), flush=True)
        finally:
            eng.close()


def test_zeroing_bookkeeping_on_every_net(gpu_device, tmp_path):
    """run_backward's on-demand zeroing (need / wrote) at every shape of the catalogue: the interleaved layerwise calls (descending, ascending, staggered) of every net, in
    one mode per net, in three child processes -- default, XFR_POISON_G=1 (the gradient region NaN-filled first: a row the bookkeeping misses
    surfaces), XFR_EAGER_ZERO=1 (the whole-region fill) -- give the same bytes per net, all finite.  The switches are latched at first use, hence children."""
    jobs = []
    for case in L.CASES:
        mode = NET_MODE[case.name]
        calls = [(F, E, V) for _, _, (F, E, V, _) in W.interleaved_calls(case, 3, mode)]
        jobs.append((case.name, mode, W.images(case, 3), calls))
    path = str(tmp_path / 'jobs.pkl')
    with open(path, 'wb') as f:
        pickle.dump(jobs, f)
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    script = 'import sys; sys.path[:0] = [%r, %r]; import test_gpu_layerwise_parity as T; T.zeroing_child(%r)' % (root, tests, path)
    digests = {}
    for tag, extra in (('default', {}), ('poisoned', {'XFR_POISON_G': '1'}), ('eager', {'XFR_EAGER_ZERO': '1'})):
        env = {k: v for k, v in os.environ.items() if k not in ('XFR_POISON_G', 'XFR_EAGER_ZERO')}
        env.update(extra)
        out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=300, env=env, cwd=root)
        assert out.returncode == 0, (tag, out.stderr[-3000:])
        lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith('DIGEST')]
        digests[tag] = {ln[1]: (ln[2], ln[3]) for ln in lines}
        assert sorted(digests[tag]) == sorted(NAMES), (tag, sorted(digests[tag]))
    bad = ['%s: default %s poisoned %s eager %s' % (nm, digests['default'][nm], digests['poisoned'][nm], digests['eager'][nm]) for nm in NAMES
           if not (digests['default'][nm] == digests['poisoned'][nm] == digests['eager'][nm] and digests['default'][nm][1] == 'finite')]
    assert not bad, 'the lazily zeroed, the poisoned and the eagerly zeroed runs differ (or hold non-finite values):\n' + '\n'.join(bad)


TAIL_NETS = ['stem', 'mfm', 'classifier', 'avg_shortcut_v4']      # P[-2] maps of 19 x 15, 37 x 31, 4 x 5 (three firings) and 16 x 24


@pytest.mark.parametrize('name', TAIL_NETS)
def test_weighted_subtree_tail(gpu_device, name):
    """Engine.weighted_subtree(output='mwp', order='engine', want_top=True), three images, topk 2 and 8 (8 exceeds the valid firings of the small nets:
    n_valid < topk), sum and max, sweep_batch None and 2.  From k_valid / w_valid / n_valid: every weight is subtree_weights' to the bit; firing 1 is
    never chosen; every chosen firing is valid (its float64 layerwise map at the engine's element and captured value has max > 0); no valid firing
    heavier than the lightest chosen one by more than 1e-4 relative is left out; slots ascend by weight; each top map and the merged map (against
    merge_truth of the float64 maps with the returned weights) obey the rule; padding slots are zero."""
    case, eng, st, nf = _setup(name, gpu_device)
    n = 3
    mode = NET_MODE[name]
    eng.set_mode(mode)
    x = W.images(case, n)
    xd = x.to(gpu_device)
    e0, e1 = W.onehot_seeds(case, n)
    ebp = W.ebp_seed(case, n)
    w_eng, idx_eng = eng.subtree_weights(xd, st, torch.stack((e0, e1), 0), True)
    cap = np.asarray(eng.ebp_capture(xd, st, ebp.unsqueeze(0), idx_eng)).reshape(nf, n)
    maps64 = [W.layerwise_truth(case, x, mode, k, idx_eng[k], cap[k], F64, _tape=W.tape(case, n, F64)).numpy() for k in range(nf)]
    maps32 = [W.layerwise_truth(case, x, mode, k, idx_eng[k], cap[k], F32, _tape=W.tape(case, n, F32)).numpy() for k in range(nf)]
    valid = np.array([[float(maps64[k][b].max()) > 0 and k != 1 for b in range(n)] for k in range(nf)])
    bad = []
    short = 0
    for topk in (2, 8):
        for do_max in (False, True):
            for sweep_batch in (None, 2):
                smap, top, w_valid, k_valid, n_valid = eng.weighted_subtree(xd, st, torch.stack((e0, e1, ebp), 0), topk, gate_ge0=True, do_max_subtree=do_max,
                                                                           output='mwp', sweep_batch=sweep_batch, order='engine', want_top=True)
                smap, top = smap.cpu().numpy(), top.cpu().numpy()
                for b in range(n):
                    tag = 'subtree/%s/top%d/%s/batch%s/sample%d' % (name, topk, 'max' if do_max else 'sum', sweep_batch, b)
                    c = int(n_valid[b])
                    ks = [int(k) for k in k_valid[b, :c]]
                    short += c < topk
                    if not (1 <= c <= topk and all(0 <= k < nf for k in ks) and len(set(ks)) == c):
                        bad.append('%s: n_valid %d, k_valid %s' % (tag, c, k_valid[b].tolist()))
                        continue
                    if not (np.all(k_valid[b, c:] == -1) and np.all(w_valid[b, c:] == 0) and np.all(top[b, c:] == 0)):
                        bad.append('%s: padding slots are not (-1, 0, zero map)' % tag)
                    if not np.array_equal(w_valid[b, :c].view(np.uint32), w_eng[ks, b].view(np.uint32)):
                        bad.append('%s: w_valid %s is not subtree_weights %s' % (tag, w_valid[b, :c].tolist(), w_eng[ks, b].tolist()))
                    if 1 in ks or not all(valid[k, b] for k in ks):
                        bad.append('%s: chosen %s, valid %s' % (tag, ks, np.nonzero(valid[:, b])[0].tolist()))
                    if np.any(np.diff(w_valid[b, :c]) < 0):
                        bad.append('%s: weights do not ascend: %s' % (tag, w_valid[b, :c].tolist()))
                    cut = float(w_valid[b, 0])
                    out = [k for k in np.nonzero(valid[:, b])[0] if int(k) not in ks and (c < topk or float(w_eng[k, b]) - cut > 1e-4 * abs(cut))]
                    if out:
                        bad.append('%s: valid firings %s (weights %s) left out; chosen %s from %.9g up' % (tag, out, w_eng[out, b].tolist(), ks, cut))
                    for t, k in enumerate(ks):
                        _rule(bad, '%s/top%d/P[%d]' % (tag, t, k), top[b, t], maps32[k][b], maps64[k][b])
                    _rule(bad, tag + '/smap', smap[b], W.merge_truth([maps32[k][b] for k in ks], w_valid[b, :c], do_max),
                          W.merge_truth([maps64[k][b] for k in ks], w_valid[b, :c], do_max))
    if name == 'classifier':
        assert short > 0, 'classifier: no call ended with n_valid < topk'
    assert not bad, '\n'.join(bad)
