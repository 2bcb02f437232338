"""Per-firing float64 parity of the engine on the nets of tests/depthwise_nets.py: a depthwise convolution behind the first layer on the vector-ALU
kernel (xfr_amd/csrc/conv_depthwise.hip, configuration 14): forward (one launch, W and relu(W) from the same staged input), backward-data (the same
kernel, Ci and Co swapped), the phases of a strided layer; which launches take that kernel (the profile records), that it agrees with the grouped
MFMA kernel (fusion-mask bit 10 keeps configuration 13), that images and channels stay apart, and that it repeats its bits.

The rule, its constants and the engine / oracle / report plumbing are tests/parity_harness.py's: for every tensor e_eng = max|engine - fp64| / max|fp64|,
e32 = max|fp32 oracle - fp64| / max|fp64|, and  e_eng <= max(4 * e32, 2e-6); the layerwise rows add the conditioning allowance of a one-element
prior (layerwise_inputs.one_element_cond).  XFR_LAYER_PARITY_REPORT=<path> writes every measured (e_eng, e32) pair there as JSON.
Measured on the MI355X over the 1038 comparisons of this file (990 per-firing and pooled, 48 layerwise and weight rows): e32 at most 9.0e-7, e_eng at
most 9.1e-7 (gdc7, norelu, the pooled P[-2] of the default schedule: e_eng 9.15e-7 against 4 x 9.05e-7), e_eng / e32 at most 7.3, on a row far
under the floor (the true-weight row of dw3_s2_odd, gate lt0, sample 2: e_eng 7.5e-8, e32 1.0e-8); the tightest comparison uses 35 % of its bound
(mult3, all, three images, P[1]: e_eng 7.09e-7 under the 2e-6 floor, 4 x e32 = 1.22e-6).  On dw_tiles, mult3_s2 and mbv1_mini configurations 13 and 14
both pass with the same margins to the printed digits.  Inputs and seeds are fixed and the kernels deterministic, so the margins repeat run to run.
"""
import os

import numpy as np
import pytest
import torch

import depthwise_nets as DN
import grouped_nets as GN
import layerwise_inputs as W
import parity_harness as H
from parity_harness import CFG_DEPTHWISE, CFG_GROUP, KEEP_ON_13, by_cfg as _by_cfg, profiled_sweep as _profiled_sweep
from xfr_amd.engine import Engine

pytestmark = pytest.mark.gpu

# one subtree mode per net for the un-observed schedules (all four across the catalogue)
SCHEDULE_MODE = {'dw_tiles': 'affineonly_with_prior', 'dw_7x7map': 'norelu', 'dw5_p2': 'all', 'dw7_p3': 'affineonly', 'gdc7': 'norelu', 'dw3_s2_odd': 'all',
                 'dw3_s2_p0': 'affineonly_with_prior', 'dw1_s2': 'affineonly', 'mult3': 'norelu', 'mult3_s2': 'all', 'dw_bias': 'affineonly_with_prior',
                 'dw_prefix': 'norelu', 'pair_g': 'affineonly', 'mbv1_mini': 'affineonly_with_prior'}
NAMES = [c.name for c in DN.CASES]
h = H.Harness(print_check=True, print_rule=True)
_engine, _oracle, _apply, _check, _rule = h.engine, h.oracle, h.apply, h.check, h.rule


@pytest.fixture(scope='module', autouse=True)
def _engines_and_report():
    yield
    h.finish('XFR_LAYER_PARITY_REPORT', merge=True)          # the other parity files write the same file earlier in a session: add to it


@pytest.mark.parametrize('name', NAMES)
def test_every_firing_matches_float64(gpu_device, name):
    """Engine.ebp_firing(k) for every firing k including k == firing_count (the P[-1] gather), four subtree modes, one and three images (three of an
    engine of max_batch 8)."""
    H.run_every_firing(h, DN.BY_NAME[name], gpu_device)


@pytest.mark.parametrize('name', NAMES)
def test_schedule_pooled_matches_float64(gpu_device, name):
    """Engine.ebp(want_pooled=True), the un-observed sweep, against the float64 pooled P[-2]: the default schedule at three and four images, fusion
    off, fusion with its optional bits off, the literal schedule at four images, and for the strided nets the phases in a row (bit 9)."""
    case = DN.BY_NAME[name]
    schedules = H.SCHEDULES + ([('phases_in_a_row', 3, {'fusion': 3 | 512})] if case.grouped[7] == 2 and case.grouped[6] > 1 else [])
    H.run_schedule_pooled(h, case, gpu_device, SCHEDULE_MODE[name], schedules)


@pytest.mark.parametrize('name', ['dw_tiles', 'mult3_s2', 'mbv1_mini'])
def test_both_kernels_pass_the_float64_rule(gpu_device, name):
    """Fusion-mask bit 10 keeps the depthwise launches on configuration 13: with it and without it every firing passes the rule (the two kernels sum in
    different orders, so they are held to the float64 truth, not to each other's bits)."""
    case = DN.BY_NAME[name]
    mode = SCHEDULE_MODE[name]
    eng = _engine(case, gpu_device)
    eng.set_mode(mode)
    st = case.program().marks['classify']
    x, seed, P32, P64 = _oracle(case, 3, mode, 0)
    xd, sd = x.to(gpu_device), seed.to(gpu_device)
    bad = []
    try:
        for tag, mask in (('cfg13', 3 | KEEP_ON_13), ('cfg14', 3)):
            eng.set_epilogue_fusion(mask)
            for k in range(eng.firing_count(st) + 1):
                _check(bad, '%s/%s/%s/P[%d]' % (name, mode, tag, k), eng.ebp_firing(xd, st, sd, k), P32[k], P64[k])
    finally:
        _apply(eng, {})
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name', ['dw3_s2_odd', 'dw_prefix'])
def test_layerwise_map_per_firing(gpu_device, name):
    """A layerwise map per firing (element slot 0 of every firing that has one) through layerwise_inputs, in calls of ascending firings -- the prefix
    launches: a gradient stream is idle above its prior, so the depthwise backward launch covers a batch prefix (in_nb > NB) -- and one call in
    descending order, three images, under the layerwise rule."""
    case = DN.BY_NAME[name]
    mode = 'affineonly_with_prior'
    eng = _engine(case, gpu_device)
    eng.set_mode(mode)
    st = case.program().marks['classify']
    n = 3
    elems, vals = W.element_table(case, n, mode)
    live = [k for k in range(elems.shape[0]) if (elems[k, 0] >= 0).all()]
    assert len(live) >= 4
    x = W.images(case, n).to(gpu_device)
    bad = []
    calls = [live[i:i + 4] for i in range(0, len(live), 4)] + [list(reversed(live[:4]))]
    for ci, order in enumerate(calls):
        F = np.array([[k] * n for k in order], dtype=np.int32)
        E = np.stack([elems[k, 0] for k in order]).astype(np.int32)
        V = np.stack([vals[k, 0] for k in order]).astype(np.float32)
        maps = eng.layerwise(x, st, F, E, V).cpu()
        for j, k in enumerate(order):
            m64, cond = W.layerwise_map_cond(case, n, mode, k, 0, torch.float64)
            m32 = W.layerwise_map(case, n, mode, k, 0, torch.float32)
            for b in range(n):
                _rule(bad, 'layerwise/%s/%s/call%d/P[%d]/sample%d' % (name, mode, ci, k, b), maps[j, b], m32[b], m64[b], cond[b])
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name', ['dw3_s2_odd', 'dw_prefix'])
def test_true_weight_pass_through_the_depthwise_layer(gpu_device, name):
    """Engine.subtree_weights (the weighted-subtree pass: true-weight gradients, the depthwise layer's true packs, by phases for the strided net) at
    three images, both gates: w per sample over the firings under the rule, idx equal to the float64 first argmax in every clear row."""
    case = DN.BY_NAME[name]
    eng = _engine(case, gpu_device)
    eng.set_mode(SCHEDULE_MODE[name])
    st = case.program().marks['classify']
    n = 3
    x = W.images(case, n).to(gpu_device)
    seed = torch.stack(W.onehot_seeds(case, n), 0)
    bad = []
    for gate in (True, False):
        t64, t32 = W.weights(case, n, gate, torch.float64), W.weights(case, n, gate, torch.float32)
        w, idx = eng.subtree_weights(x, st, seed, gate)
        assert w.shape == idx.shape == t64['w'].shape, (w.shape, t64['w'].shape)
        for b in range(n):
            _rule(bad, 'weights/%s/%s/sample%d' % (name, 'ge0' if gate else 'lt0', b), torch.as_tensor(w[:, b]), t32['w'][:, b], t64['w'][:, b], 0.0)
        for k in range(w.shape[0]):
            for b in range(n):
                if t64['clear'][k, b] and int(idx[k, b]) != int(t64['idx'][k, b]):
                    bad.append('firing %d sample %d (clear, gap %.2e): idx %d, fp64 %d' % (k, b, t64['gap'][k, b], int(idx[k, b]), int(t64['idx'][k, b])))
    assert not bad, '\n'.join(bad)


# -- launch records -----------------------------------------------------------------------------------------------------------------------------
def test_depthwise_launch_records(gpu_device, tmp_path):
    """A sweep of dw_bias over two seeds of three images: exactly one forward launch of configuration 14 (W and relu(W) in one launch, K 9,
    M = 3 x 9 x 12), one backward-data launch over both gradient streams (M twice that), and no launch of configuration 13."""
    case = DN.BY_NAME['dw_bias']
    eng = _engine(case, gpu_device)
    eng.set_mode('norelu')
    rows = _profiled_sweep(eng, case, gpu_device, str(tmp_path / 'dw_bias.csv'), 3, 2)
    dw = _by_cfg(rows, CFG_DEPTHWISE)
    assert len(rows) > len(dw) == 2, rows
    assert dw[0] == [20, 2, 9, 3 * 9 * 12, 3, 1, 1, 0, 0], dw
    assert dw[1] == [20, 1, 9, 2 * 3 * 9 * 12, 3, 1, 1, 0, 0], dw
    assert not _by_cfg(rows, CFG_GROUP), rows


def test_phase_launch_records(gpu_device, tmp_path):
    """dw3_s2_odd: the strided forward and the four phases of its backward-data pass on configuration 14, with the K and M of grouped_nets.phases."""
    case = DN.BY_NAME['dw3_s2_odd']
    eng = _engine(case, gpu_device)
    eng.set_mode('norelu')
    rows = _profiled_sweep(eng, case, gpu_device, str(tmp_path / 'dw3_s2_odd.csv'), 3, 2)
    dw = _by_cfg(rows, CFG_DEPTHWISE)
    assert not _by_cfg(rows, CFG_GROUP), rows
    want = GN.phases(case)
    assert len(dw) == 1 + len(want) == 5, rows
    assert dw[0] == [16, 2, 9, 3 * 7 * 5, 3, 2, 1, 0, 0], dw
    for r, ph in zip(dw[1:], want):
        assert r == [16, 1, ph['K'], 2 * 3 * ph['nq'] * ph['nu'], ph['ka'], 1, 2, 0, 1], (r, ph)
    assert [ph['K'] for ph in want] == [4, 2, 2, 1]


def test_multiplier_launch_records(gpu_device, tmp_path):
    """mult3: Ci 1, Co 3 forward (K 9, 24 output channels), Ci 3, Co 1 backward (K 27, 8 output channels), both on configuration 14."""
    case = DN.BY_NAME['mult3']
    eng = _engine(case, gpu_device)
    eng.set_mode('norelu')
    rows = _profiled_sweep(eng, case, gpu_device, str(tmp_path / 'mult3.csv'), 3, 2)
    dw = _by_cfg(rows, CFG_DEPTHWISE)
    assert not _by_cfg(rows, CFG_GROUP), rows
    assert dw == [[24, 2, 9, 3 * 10 * 7, 3, 1, 1, 0, 0], [8, 1, 27, 2 * 3 * 10 * 7, 3, 1, 1, 0, 0]], rows


def test_what_stays_on_the_grouped_kernel(gpu_device, tmp_path):
    """pair_g (Ci = Co = 2) and grouped_nets' g8_c4 (Ci = Co = 4) launch configuration 13 only; so does dw_bias with fusion-mask bit 10 set."""
    for case in (DN.BY_NAME['pair_g'], GN.BY_NAME['g8_c4']):
        e = Engine(case.program(), 4, gpu_device)
        try:
            e.load_weights(case.params())
            e.set_mode('norelu')
            rows = _profiled_sweep(e, case, gpu_device, str(tmp_path / (case.name + '.csv')), 3, 2)
        finally:
            e.close()
        assert len(_by_cfg(rows, CFG_GROUP)) == 2 and not _by_cfg(rows, CFG_DEPTHWISE), (case.name, rows)
    case = DN.BY_NAME['dw_bias']
    eng = _engine(case, gpu_device)
    eng.set_mode('norelu')
    try:
        eng.set_epilogue_fusion(3 | KEEP_ON_13)
        rows = _profiled_sweep(eng, case, gpu_device, str(tmp_path / 'dw_bias_13.csv'), 3, 2)
    finally:
        _apply(eng, {})
    g = _by_cfg(rows, CFG_GROUP)
    assert not _by_cfg(rows, CFG_DEPTHWISE), rows
    assert g == [[20, 2, 9, 3 * 9 * 12, 3, 1, 1, 0, 0], [20, 1, 9, 2 * 3 * 9 * 12, 3, 1, 1, 0, 0]], rows


# -- isolation ----------------------------------------------------------------------------------------------------------------------------------
def _isolation_params(case, c_in, c_hot):
    """The case's parameters with signs arranged so that a huge value at input channel c_in drives channel c_hot of the first layer up and every
    other channel down (below the ReLU: zero), and channel c_hot of the depthwise layer down: the poison lives in one channel of the depthwise
    layer's input and output and nowhere behind its ReLU."""
    p = {k: v.clone() for k, v in case.params().items()}
    w = p['conv0.weight']
    w[:, c_in] = -w[:, c_in].abs() - 0.01
    w[c_hot, c_in] = w[c_hot, c_in].abs()
    p['gconv.weight'][c_hot] = -p['gconv.weight'][c_hot].abs() - 0.01
    return p


def test_images_and_channels_stay_apart(gpu_device):
    """dw_7x7map at three images, mode `all`, the three images of a channel in one tile of the kernel.  One input element of image 0 is +inf; the run
    it is compared with has 1e30 there (finite all the way).  Either value is far below zero behind the first layer's BatchNorm in every channel but
    one, so the depthwise layer sees the poison in ONE channel of image 0.  Its forward output is non-finite there, and has the bits of the finite
    run in the other channels of image 0 and in images 1 and 2; every firing keeps its bits in images 1 and 2, and the firing on the depthwise
    layer's output keeps them in the other channels of image 0.  Then the same with the poison in the gradient: a seed with one inf entry for image 0."""
    case = DN.BY_NAME['dw_7x7map']
    prog = case.program()
    st = prog.marks['classify']
    gop = case.grouped_op(prog)
    c_in, c_hot = 2, 5
    others = [c for c in range(16) if c != c_hot]
    eng = Engine(prog, 8, gpu_device)
    try:
        eng.load_weights(_isolation_params(case, c_in, c_hot))
        eng.set_mode('all')
        x, seed, _, _ = _oracle(case, 3, 'all', 0)
        big, hot = x.clone(), x.clone()
        big[0, c_in, 3, 3] = 1e30
        hot[0, c_in, 3, 3] = float('inf')
        big, hot, sd = big.to(gpu_device), hot.to(gpu_device), seed.to(gpu_device)
        a, b = eng.forward(big, gop + 1).cpu(), eng.forward(hot, gop + 1).cpu()
        assert bool(torch.isfinite(a).all())
        assert not bool(torch.isfinite(b[0, c_hot]).all())                    # the poison did arrive
        assert bool(torch.isfinite(b[0, others]).all()) and torch.equal(a[0, others], b[0, others])
        assert torch.equal(a[1:], b[1:])
        names = prog.layernames('all', st)
        at_output = [k for k, nm in enumerate(names) if 'groups=16' in nm][0] - 1          # the firing of the op that reads the depthwise layer's output
        nf = eng.firing_count(st)
        for k in range(nf + 1):
            pa, pb = eng.ebp_firing(big, st, sd, k).cpu(), eng.ebp_firing(hot, st, sd, k).cpu()
            assert bool(torch.isfinite(pa[1:]).all()) and torch.equal(pa[1:], pb[1:]), k
            if k == at_output:
                assert tuple(pa.shape[1:]) == (16, 7, 7)
                assert bool(torch.isfinite(pb[0, others]).all()) and torch.equal(pa[0, others], pb[0, others])
        # the gradient
        xd = x.to(gpu_device)
        hot_seed = seed.clone()
        hot_seed[0, 0, 1] = float('inf')
        hs = hot_seed.to(gpu_device)
        poisoned = 0
        for k in range(nf + 1):
            pa, pb = eng.ebp_firing(xd, st, sd, k).cpu(), eng.ebp_firing(xd, st, hs, k).cpu()
            assert bool(torch.isfinite(pb[1:]).all()) and torch.equal(pa[1:], pb[1:]), k
            poisoned += 0 if bool(torch.isfinite(pb[0]).all()) else 1
        assert poisoned >= 1
    finally:
        eng.close()


def test_unreached_pixels_get_zero_gradient(gpu_device):
    """dw3_s2_p0: no window of the 3x3 / s2 / p0 depthwise layer reads input row 11 or column 9; after a first sweep in another mode has left other
    values in the workspace, the P of every hook on that tensor is exactly zero there."""
    case = DN.BY_NAME['dw3_s2_p0']
    eng = _engine(case, gpu_device)
    st = case.program().marks['classify']
    x0, seed0, _, _ = _oracle(case, 3, 'all', 1)
    eng.set_mode('all')
    for k in range(eng.firing_count(st)):
        eng.ebp_firing(x0.to(gpu_device), st, seed0.to(gpu_device), k)
    eng.set_mode('norelu')
    x, seed, _, P64 = _oracle(case, 3, 'norelu', 0)
    hits = 0
    for k in range(eng.firing_count(st)):
        if tuple(P64[k].shape[2:]) != (12, 10):
            continue
        if not (float(P64[k][:, :, 11].abs().max()) == 0 and float(P64[k][:, :, :, 9].abs().max()) == 0):
            continue              # (the first layer's own hooks below the ReLU see the 3x3 of conv0's backward: not this tensor)
        got = eng.ebp_firing(x.to(gpu_device), st, seed.to(gpu_device), k).cpu()
        assert float(got[:, :, 11].abs().max()) == 0 and float(got[:, :, :, 9].abs().max()) == 0, k
        assert float(got.abs().max()) > 0
        hits += 1
    assert hits >= 1


def test_two_sweeps_are_bit_identical(gpu_device):
    """mbv1_mini at four images: no atomics in the depthwise launches, one summation order, the phases write disjoint pixels."""
    case = DN.BY_NAME['mbv1_mini']
    eng = _engine(case, gpu_device)
    mode = SCHEDULE_MODE['mbv1_mini']
    eng.set_mode(mode)
    st = case.program().marks['classify']
    x, seed, _, _ = _oracle(case, 4, mode, 1)
    x, seed = x.to(gpu_device), seed.to(gpu_device)
    runs = []
    for _ in range(2):
        pooled = eng.ebp(x, st, seed, want_mwp=False, want_pooled=True)[1].cpu()
        fired = [eng.ebp_firing(x, st, seed, k).cpu() for k in range(eng.firing_count(st))]
        runs.append((pooled, fired))
    assert bool(torch.isfinite(runs[0][0]).all()) and float(runs[0][0].abs().max()) > 0
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(u, v) for u, v in zip(runs[0][1], runs[1][1]))


@pytest.mark.parametrize('mode', ('affineonly_with_prior', 'norelu'))
def test_mini_mobilenet_matches_live_reference_golden(gpu_device, mode):
    """models/mobilenet.py (alpha 0.25, two pairs, the global depthwise head on a 10 x 9 map, 3 x 40 x 36) behind WhiteboxTVResnet against what the
    live reference computed for the plain-torch twin (tests/golden/golden_depthwise.npz): per-firing P sums and names, pooled P[-2] and the final map
    of `ebp` on the hooked `fc`, and the triplet contrastive map, with the tolerances of test_mini_resnext_matches_live_reference_golden."""
    import depthwise_golden_inputs as G
    from parity_utils import MAP_RTOL_CONTRAST, assert_map_close, assert_trace_close
    from xfr_amd.models import whitebox as WB
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', G.GOLDEN))
    bb, _ = G.mini_backbone()
    bb.to(gpu_device)
    x = G.image()
    wbn = WB.WhiteboxTVResnet(bb)
    wb = WB.Whitebox(wbn, ebp_subtree_mode=mode)
    wb.debug_trace = True
    try:
        Pn = G.class_seed(3, G.NUM_CLASSES)
        pooled = wb.ebp(x, Pn, mwp=True)
        assert_trace_close(np.asarray(wb.P_trace)[:, 0], wb.P_layername, gold['%s/ebp/sums' % mode], gold['%s/ebp/names' % mode], '%s ebp trace' % mode)
        assert list(wb.P_layername) == [str(v) for v in gold['%s/ebp/layernames' % mode]]
        assert_map_close(pooled, gold['%s/ebp/pooled' % mode], '%s ebp pooled P[-2]' % mode)
        wb.debug_trace = False
        assert_map_close(wb.ebp(x, Pn), gold['%s/ebp/map' % mode], '%s ebp map' % mode)
        enc = wbn.encode(x.to(gpu_device))
        assert tuple(enc.shape) == (1, G.FEATURES)
        wbn.set_triplet_classifier(*G.triplet_rows())
        assert wbn.num_classes() == 2
        assert_map_close(wb.contrastive_ebp(x, 0, 1), gold['%s/triplet/map' % mode], '%s triplet map' % mode, rtol=MAP_RTOL_CONTRAST)
        assert_map_close(wb.ebp(x, G.class_seed(1, 2), mwp=True), gold['%s/triplet/pooled' % mode], '%s triplet pooled P[-2]' % mode)
    finally:
        wbn.engine().close()
