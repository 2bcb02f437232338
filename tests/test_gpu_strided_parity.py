"""Per-firing float64 parity of the engine on the nets of tests/strided_nets.py: a strided KxK convolution behind the first layer, whose
backward-data pass runs as one stride-1 GEMM per phase, scattered onto a zero-filled gradient tensor (xfr_amd/csrc/plan.hip PhaseRec,
backward.hip bwd_conv_params).

The rule, its constants and the engine / oracle / report plumbing are tests/parity_harness.py's: for every tensor  e_eng = max|engine - fp64| / max|fp64|,
e32 = max|fp32 oracle - fp64| / max|fp64|, and  e_eng <= max(4 * e32, 2e-6).  The layerwise rows add the conditioning allowance of a one-element
prior (layerwise_inputs.one_element_cond).
XFR_LAYER_PARITY_REPORT=<path> writes every measured (e_eng, e32) pair there as JSON.
Measured on the MI355X over the 531 per-firing and pooled comparisons of this file: e32 between 8.6e-8 and 2.4e-6, e_eng at most 2.2e-6, e_eng / e32 at
most 3.9; the tightest comparison uses 98 % of its bound (basic_block, mode all, one image, P[2]: e_eng 2.21e-6 against 4 x 5.64e-7).  Inputs and seeds
are fixed and the kernels deterministic, so the margins repeat run to run.
"""
import hashlib
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import layerwise_inputs as W
import parity_harness as H
import strided_nets as S
from xfr_amd.engine import Engine

pytestmark = pytest.mark.gpu

# one subtree mode per net for the un-observed schedules (all four across the catalogue)
SCHEDULE_MODE = {'s2_odd': 'affineonly_with_prior', 's2_valid': 'norelu', 'basic_block': 'all', 'bottleneck_v15': 'affineonly', 's3_5x5': 'norelu',
                 'patch2': 'all', 'mid7': 'affineonly_with_prior'}
NAMES = [c.name for c in S.CASES]
h = H.Harness(print_check=True)
_engine, _oracle, _rule = h.engine, h.oracle, h.rule


@pytest.fixture(scope='module', autouse=True)
def _engines_and_report():
    yield
    h.finish('XFR_LAYER_PARITY_REPORT', merge=True)          # test_gpu_layer_parity.py writes the same file earlier in a session: add to it


@pytest.mark.parametrize('name', NAMES)
def test_every_firing_matches_float64(gpu_device, name):
    """Engine.ebp_firing(k) for every firing k including k == firing_count (the P[-1] gather), four subtree modes, one and three images."""
    H.run_every_firing(h, S.BY_NAME[name], gpu_device)


def test_unread_rows_get_zero_gradient(gpu_device):
    """s2_valid: no window of the 3x3/s2/p0 layer reads input row 9 or column 7; the P of every hook on that tensor is exactly zero there."""
    case = S.BY_NAME['s2_valid']
    eng = _engine(case, gpu_device)
    st = case.program().marks['classify']
    eng.set_mode('norelu')
    x, seed, _, P64 = _oracle(case, 3, 'norelu', 0)
    hits = 0
    for k in range(eng.firing_count(st)):
        if tuple(P64[k].shape[2:]) != (10, 8):
            continue
        if not (float(P64[k][:, :, 9].abs().max()) == 0 and float(P64[k][:, :, :, 7].abs().max()) == 0):
            continue              # (the first layer's own hooks below the ReLU see the 3x3 of conv0's backward: not this tensor)
        got = eng.ebp_firing(x.to(gpu_device), st, seed.to(gpu_device), k).cpu()
        assert float(got[:, :, 9].abs().max()) == 0 and float(got[:, :, :, 7].abs().max()) == 0, k
        assert float(got.abs().max()) > 0
        hits += 1
    assert hits >= 1


@pytest.mark.parametrize('name', NAMES)
def test_schedule_pooled_matches_float64(gpu_device, name):
    """Engine.ebp(want_pooled=True), the un-observed sweep, against the float64 pooled P[-2]: the default schedule at three and four images (lean where
    it applies), fusion off, fusion with its optional bits off, and the literal schedule at four images."""
    H.run_schedule_pooled(h, S.BY_NAME[name], gpu_device, SCHEDULE_MODE[name], H.SCHEDULES)


def test_layerwise_priors_around_the_strided_layer(gpu_device):
    """basic_block: one layerwise call of two sweeps, the prior of the first at the hook of the 3x3/s2 layer's OUTPUT (above it: the sweep runs
    through the phases and the projection's scatter), the prior of the second at the first hook of the block's INPUT tensor (below it: that stream
    is idle while the strided GEMMs run, prefix launches), three images, against the float64 tape under the layerwise rule."""
    case = S.BY_NAME['basic_block']
    mode = 'affineonly_with_prior'
    eng = _engine(case, gpu_device)
    eng.set_mode(mode)
    prog = case.program()
    st = prog.marks['classify']
    n = 3
    ops = prog.firing_ops(mode, st)
    conv1 = [i for i, o in enumerate(prog.ops) if o.w_weight >= 0 and prog.weight_names[o.w_weight] == 'b.conv1.weight'][0]
    bn1 = conv1 + 1
    above, below = ops.index(bn1), ops.index(conv1)           # BatchNorm hook on the strided layer's output; the strided layer's own hook on its input
    assert above < below
    elems, vals = W.element_table(case, n, mode)
    assert (elems[above, 0] >= 0).all() and (elems[below, 0] >= 0).all()
    x = W.images(case, n).to(gpu_device)
    bad = []
    for order in ((above, below), (below, above)):            # ascending firings: prefix launches; descending: whole launches
        F = np.array([[k] * n for k in order], dtype=np.int32)
        E = np.stack([elems[k, 0] for k in order]).astype(np.int32)
        V = np.stack([vals[k, 0] for k in order]).astype(np.float32)
        maps = eng.layerwise(x, st, F, E, V).cpu()
        for j, k in enumerate(order):
            m64, cond = W.layerwise_map_cond(case, n, mode, k, 0, torch.float64)
            m32 = W.layerwise_map(case, n, mode, k, 0, torch.float32)
            for b in range(n):
                _rule(bad, 'layerwise/basic_block/%s/order%d.%d/P[%d]/sample%d' % (mode, order[0], order[1], k, b), maps[j, b], m32[b], m64[b], cond[b])
    assert not bad, '\n'.join(bad)


def poisoned_child(path):
    """Child process of test_poisoned_gradient_region: the layerwise calls read from `path` on s2_valid, one sha256."""
    with open(path, 'rb') as f:
        mode, x, calls = pickle.load(f)
    dev = torch.device('cuda', 0)
    case = S.BY_NAME['s2_valid']
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
        print('DIGEST %s %s' % (h.hexdigest(), 'finite' if finite else 'NONFINITE'), flush=True)
    finally:
        eng.close()


def test_poisoned_gradient_region(gpu_device, tmp_path):
    """s2_valid with the gradient region NaN-filled before every layerwise sweep (XFR_POISON_G=1, latched at first use, hence a child process): the
    pixels no phase writes and the rows of idle streams read the zero fill, not the poison -- the maps equal this process's bit for bit and are finite."""
    case = S.BY_NAME['s2_valid']
    mode = SCHEDULE_MODE['s2_valid']
    calls = [(F, E, V) for _, _, (F, E, V, _) in W.interleaved_calls(case, 3, mode)]
    x = W.images(case, 3)
    eng = _engine(case, gpu_device)
    eng.set_mode(mode)
    st = case.program().marks['classify']
    h = hashlib.sha256()
    for (F, E, V) in calls:
        m = eng.layerwise(x.to(gpu_device), st, F, E, V).cpu().numpy()
        assert np.isfinite(m).all()
        h.update(np.ascontiguousarray(m, dtype=np.float32).tobytes())
    path = str(tmp_path / 'calls.pkl')
    with open(path, 'wb') as f:
        pickle.dump((mode, x, calls), f)
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    script = 'import sys; sys.path[:0] = [%r, %r]; import test_gpu_strided_parity as T; T.poisoned_child(%r)' % (root, tests, path)
    env = {k: v for k, v in os.environ.items() if k not in ('XFR_POISON_G', 'XFR_EAGER_ZERO')}
    env['XFR_POISON_G'] = '1'
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=120, env=env, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith('DIGEST')]
    assert lines == [['DIGEST', h.hexdigest(), 'finite']], (lines, h.hexdigest())


@pytest.mark.parametrize('mode', ('affineonly_with_prior', 'norelu'))
def test_tv_resnet_matches_live_reference_golden(gpu_device, mode):
    """models/tv_resnet.py (BasicBlock [1, 1, 1, 1], width 16, 3 x 40 x 36) behind WhiteboxTVResnet against what the live reference computed for the
    plain-torch twin (tests/golden/golden_strided.npz): per-firing P sums and names, pooled P[-2] and the final map of `ebp` on the hooked `fc`, and
    the triplet contrastive map, with the tolerances tests/parity_utils.py gives mini nets."""
    import strided_golden_inputs as G
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
        assert_map_close(pooled, gold['%s/ebp/pooled' % mode], '%s ebp pooled P[-2]' % mode)
        wb.debug_trace = False
        assert_map_close(wb.ebp(x, Pn), gold['%s/ebp/map' % mode], '%s ebp map' % mode)
        enc = wbn.encode(x.to(gpu_device))
        assert tuple(enc.shape) == (1, 128)
        wbn.set_triplet_classifier(*G.triplet_rows())
        assert wbn.num_classes() == 2
        assert_map_close(wb.contrastive_ebp(x, 0, 1), gold['%s/triplet/map' % mode], '%s triplet map' % mode, rtol=MAP_RTOL_CONTRAST)
        assert_map_close(wb.ebp(x, G.class_seed(1, 2), mwp=True), gold['%s/triplet/pooled' % mode], '%s triplet pooled P[-2]' % mode)
    finally:
        wbn.engine().close()


@pytest.mark.parametrize('name', ['basic_block', 's3_5x5', 'mid7'])
def test_true_weight_pass_through_the_phases(gpu_device, name):
    """Engine.subtree_weights (the weighted-subtree pass: true-weight gradients, the phases' true packs) at three images, both gates: w per sample over
    the firings under the rule, idx equal to the float64 first argmax in every clear row (layerwise_inputs.weight_truth)."""
    case = S.BY_NAME[name]
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
        assert w.shape == idx.shape == t64['w'].shape, (name, w.shape, t64['w'].shape)
        for b in range(n):
            _rule(bad, 'weights/%s/%s/sample%d' % (name, 'ge0' if gate else 'lt0', b), torch.as_tensor(w[:, b]), t32['w'][:, b], t64['w'][:, b], 0.0)
        for k in range(w.shape[0]):
            for b in range(n):
                if t64['clear'][k, b] and int(idx[k, b]) != int(t64['idx'][k, b]):
                    bad.append('%s: firing %d sample %d (clear, gap %.2e): idx %d, fp64 %d' % (name, k, b, t64['gap'][k, b], int(idx[k, b]), int(t64['idx'][k, b])))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name', ['basic_block', 's3_5x5'])
def test_phases_side_by_side_equal_in_a_row_bits(gpu_device, name):
    """The phase launches of one layer run side by side on side streams (they write disjoint pixels); fusion-mask bit 9 runs them one after another.
    Same launches, so the pooled P[-2] and every firing's tensor are the same bits (s3_5x5: nine phases over the sweep's stream and three side streams)."""
    case = S.BY_NAME[name]
    eng = _engine(case, gpu_device)
    mode = SCHEDULE_MODE[name]
    eng.set_mode(mode)
    st = case.program().marks['classify']
    x, seed, _, _ = _oracle(case, 3, mode, 1)
    x, seed = x.to(gpu_device), seed.to(gpu_device)
    got = {}
    try:
        for tag, mask in (('side_by_side', 3), ('in_a_row', 3 | 512)):
            eng.set_epilogue_fusion(mask)
            pooled = [eng.ebp(x, st, seed, want_mwp=False, want_pooled=True)[1].cpu() for _ in range(3)]
            fired = [eng.ebp_firing(x, st, seed, k).cpu() for k in range(eng.firing_count(st))]
            assert all(torch.equal(pooled[0], p) for p in pooled[1:]), tag
            got[tag] = (pooled[0], fired)
    finally:
        eng.set_epilogue_fusion(3)
    assert bool(torch.isfinite(got['in_a_row'][0]).all()) and float(got['in_a_row'][0].abs().max()) > 0
    assert torch.equal(got['side_by_side'][0], got['in_a_row'][0])
    assert all(torch.equal(u, v) for u, v in zip(got['side_by_side'][1], got['in_a_row'][1]))
