"""Per-firing float64 parity of the engine on the nets of tests/grouped_nets.py: a grouped convolution behind the first layer, forward (one launch,
W and relu(W) from the same staged input), backward-data (the same kernel, Ci and Co swapped) and, for a strided grouped 3x3, the phases
(xfr_amd/csrc/conv_group.hip, plan.hip, backward.hip).

The rule, its constants and the engine / oracle / report plumbing are tests/parity_harness.py's: for every tensor
e_eng = max|engine - fp64| / max|fp64|, e32 = max|fp32 oracle - fp64| / max|fp64|, and  e_eng <= max(4 * e32, 2e-6).  The layerwise rows add the
conditioning allowance of a one-element prior (layerwise_inputs.one_element_cond).
XFR_LAYER_PARITY_REPORT=<path> writes every measured (e_eng, e32) pair there as JSON.
Measured on the MI355X over the 677 comparisons of this file (614 per-firing and pooled, 63 layerwise and weight rows): e32 at most 7.4e-7, e_eng at
most 1.4e-6, e_eng / e32 at most 3.6 (g2_ragged, norelu, three images, P[5]: e_eng 1.33e-6 against 4 x 3.71e-7); the tightest comparison uses 69 % of its
bound (g2_ragged, norelu, three images, P[4]: e_eng 1.38e-6 under the 2e-6 floor, 4 x e32 = 1.75e-6).  Inputs and seeds are fixed and the kernels
deterministic, so the margins repeat run to run.
"""
import os

import numpy as np
import pytest
import torch

import grouped_nets as GN
import layer_nets as L
import layerwise_inputs as W
import parity_harness as H
from xfr_amd.engine import Engine

pytestmark = pytest.mark.gpu

# one subtree mode per net for the un-observed schedules (all four across the catalogue)
SCHEDULE_MODE = {'g8_c4': 'affineonly_with_prior', 'depthwise': 'norelu', 'dw_mult2': 'all', 'g2_ragged': 'affineonly', 'g3_odd': 'norelu',
                 'g4_1x1_s2': 'all', 'g4_5x5_bias': 'affineonly_with_prior', 'resnext_block': 'affineonly_with_prior', 'g2_prefix': 'norelu'}
NAMES = [c.name for c in GN.CASES]
h = H.Harness(print_check=True, print_rule=True)
_engine, _oracle, _rule = h.engine, h.oracle, h.rule


@pytest.fixture(scope='module', autouse=True)
def _engines_and_report():
    yield
    h.finish('XFR_LAYER_PARITY_REPORT', merge=True)          # the other parity files write the same file earlier in a session: add to it


@pytest.mark.parametrize('name', NAMES)
def test_every_firing_matches_float64(gpu_device, name):
    """Engine.ebp_firing(k) for every firing k including k == firing_count (the P[-1] gather), four subtree modes, one and three images (three of an
    engine of max_batch 8)."""
    H.run_every_firing(h, GN.BY_NAME[name], gpu_device)


@pytest.mark.parametrize('name', NAMES)
def test_schedule_pooled_matches_float64(gpu_device, name):
    """Engine.ebp(want_pooled=True), the un-observed sweep, against the float64 pooled P[-2]: the default schedule at three and four images (lean on the
    dense neighbours where it applies, the grouped layer literal), fusion off, fusion with its optional bits off, the literal schedule at four images,
    and for resnext_block the phases in a row (bit 9)."""
    schedules = H.SCHEDULES + ([('phases_in_a_row', 3, {'fusion': 3 | 512})] if name == 'resnext_block' else [])
    H.run_schedule_pooled(h, GN.BY_NAME[name], gpu_device, SCHEDULE_MODE[name], schedules)


def test_groups_do_not_mix(gpu_device):
    """g8_c4, norelu: one input channel of group 0 of the grouped layer is made infinite (the beta of the BatchNorm in front of it).  The forward output
    of the grouped layer and the P of every firing stay finite, and the same bits as with a finite beta, in the channels of groups 1 .. 7: no K step is
    shared between groups, so no 0 x inf reaches them.  (The P[-1] gather lies behind the dense first layer, which mixes all channels by definition.)"""
    case = GN.BY_NAME['g8_c4']
    prog = case.program()
    st = prog.marks['classify']
    gout = case.grouped_op(prog) + 1
    x, seed, _, _ = _oracle(case, 3, 'norelu', 0)
    xd, sd = x.to(gpu_device), seed.to(gpu_device)
    clean = _engine(case, gpu_device)
    clean.set_mode('norelu')
    params = {k: v.clone() for k, v in case.params().items()}
    params['bn0.bias'][1] = float('inf')
    hot = Engine(prog, 8, gpu_device)
    try:
        hot.load_weights(params)
        hot.set_mode('norelu')
        a, b = clean.forward(xd, gout).cpu(), hot.forward(xd, gout).cpu()
        assert not bool(torch.isfinite(b[:, :4]).all())                       # the poison did arrive in group 0
        assert bool(torch.isfinite(b[:, 4:]).all()) and torch.equal(a[:, 4:], b[:, 4:])
        nf = clean.firing_count(st)
        poisoned = 0
        for k in range(nf):
            pa, pb = clean.ebp_firing(xd, st, sd, k).cpu(), hot.ebp_firing(xd, st, sd, k).cpu()
            assert pa.shape[1] == 32, (k, tuple(pa.shape))
            assert bool(torch.isfinite(pb[:, 4:]).all()), k
            assert torch.equal(pa[:, 4:], pb[:, 4:]), k
            poisoned += 0 if bool(torch.isfinite(pb[:, :4]).all()) else 1
        assert poisoned >= 1
    finally:
        hot.close()


def test_dense_sized_weight_is_refused(gpu_device):
    """A grouped layer's weight view must hold cout x Ci x kh x kw elements: the dense size is refused by the pack path with both numbers."""
    case = GN.BY_NAME['g8_c4']
    params = dict(case.params())
    params['gconv.weight'] = torch.zeros((32, 32, 3, 3))
    eng = Engine(case.program(), 2, gpu_device)
    try:
        with pytest.raises(ValueError, match=r'weight has 9216 elements, expected 1152'):
            eng.load_weights(params)
    finally:
        eng.close()


def test_two_sweeps_are_bit_identical(gpu_device):
    """resnext_block at four images: no atomics anywhere in the grouped launches, the phases write disjoint pixels."""
    case = GN.BY_NAME['resnext_block']
    eng = _engine(case, gpu_device)
    mode = SCHEDULE_MODE['resnext_block']
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


@pytest.mark.parametrize('name', ['resnext_block', 'g2_prefix'])
def test_layerwise_map_per_firing(gpu_device, name):
    """A layerwise map per firing (element slot 0 of every firing that has one) through layerwise_inputs, in calls of ascending firings -- the prefix
    launches: a gradient stream is idle above its prior, so the grouped backward GEMM of g2_prefix covers a batch prefix (in_nb > NB) -- and one call
    in descending order, three images, under the layerwise rule."""
    case = GN.BY_NAME[name]
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


def test_true_weight_pass_through_the_grouped_phases(gpu_device):
    """Engine.subtree_weights on resnext_block (the weighted-subtree pass: true-weight gradients, the grouped layer's true per-group phase packs) at three
    images, both gates: w per sample over the firings under the rule, idx equal to the float64 first argmax in every clear row."""
    case = GN.BY_NAME['resnext_block']
    eng = _engine(case, gpu_device)
    eng.set_mode(SCHEDULE_MODE['resnext_block'])
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
            _rule(bad, 'weights/resnext_block/%s/sample%d' % ('ge0' if gate else 'lt0', b), torch.as_tensor(w[:, b]), t32['w'][:, b], t64['w'][:, b], 0.0)
        for k in range(w.shape[0]):
            for b in range(n):
                if t64['clear'][k, b] and int(idx[k, b]) != int(t64['idx'][k, b]):
                    bad.append('firing %d sample %d (clear, gap %.2e): idx %d, fp64 %d' % (k, b, t64['gap'][k, b], int(idx[k, b]), int(t64['idx'][k, b])))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('mode', ('affineonly_with_prior', 'norelu'))
def test_mini_resnext_matches_live_reference_golden(gpu_device, mode):
    """models/tv_resnet.py (Bottleneck [1, 1, 1, 1], width 16, groups 4, width_per_group 16, 3 x 40 x 36) behind WhiteboxTVResnet against what the live
    reference computed for the plain-torch twin (tests/golden/golden_grouped.npz): per-firing P sums and names, pooled P[-2] and the final map of `ebp` on
    the hooked `fc`, and the triplet contrastive map, with the tolerances of test_tv_resnet_matches_live_reference_golden."""
    import grouped_golden_inputs as G
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


def test_grouped_launch_counters(gpu_device, tmp_path):
    """The profile records (Cout, nhalves, K, M, kh, stride, out_stride, relu_in, accumulate, ms, TFLOP/s, cfg) of a sweep of g8_c4 over two seeds of
    three images show exactly one launch of configuration 13 for the grouped forward -- W and relu(W) in one launch, M = 3 x 15 x 13 -- and one for its
    backward-data pass over both gradient streams (M twice that), both with the K of one group; no ungrouped net of tests/layer_nets.py launches it."""
    case = GN.BY_NAME['g8_c4']
    eng = _engine(case, gpu_device)
    eng.set_mode('norelu')
    rows = H.profiled_sweep(eng, case, gpu_device, str(tmp_path / 'g8_c4.csv'), 3, 2)
    grouped = [r for r in rows if int(r[11]) == H.CFG_GROUP]
    assert len(rows) > len(grouped) == 2, rows
    fwd, bwd = grouped
    assert [int(v) for v in fwd[:9]] == [32, 2, 36, 3 * 15 * 13, 3, 1, 1, 0, 0], fwd
    assert [int(v) for v in bwd[:9]] == [32, 1, 36, 2 * 3 * 15 * 13, 3, 1, 1, 0, 0], bwd
    for other in L.CASES:
        e = Engine(other.program(), 2, gpu_device)
        try:
            e.load_weights(other.params())
            e.set_mode('affineonly_with_prior')
            rows = H.profiled_sweep(e, other, gpu_device, str(tmp_path / (other.name + '.csv')), 1, 1)
        finally:
            e.close()
        assert rows and not [r for r in rows if int(r[11]) == H.CFG_GROUP], (other.name, rows)
