"""Per-firing float64 parity of the engine on the catalogue of small layer programs (tests/layer_nets.py): every launch form the planner
picks at odd, non-square shapes -- backward-data GEMMs, stride-s scatters, dual W / relu(W) and lean two-accumulator launches, compiled
and interpreted chains, two-stream tiles, MaxFeatureMap pairs and the direct stem, bf16x6, K-parts, the P[-1] gather -- and, at the smallest
shapes that reach them, every float4 / row-pair / fused / global form of the pooling and normalize kernels, is compared
element by element with the float64 oracle tape.

The rule, for every tensor:  e_eng = max|engine - fp64| / max|fp64|,  e32 = max|fp32 oracle - fp64| / max|fp64| (the reference's own
precision on the same tensor), and  e_eng <= max(K_RATIO * e32, FLOOR); it is stated in tests/parity_harness.py, with its constants and the engine
cache and report of this and the other parity files.  Measured on the MI355X over the 1832 comparisons of this file
(e32 between 5e-8 and 4e-6, e_eng at most 5.5e-6): e_eng / e32 per firing at most 1.0 (pool_odd17) .. 5.6 (halo65), on the pooled P[-2] of the
schedule matrix at most 1.3 (pool_odd17) .. 5.9 (classifier, lean and two-stream legs); the 24 comparisons above 4 all have e_eng <= 7.7e-7, under
the floor.  K_RATIO 4 and FLOOR 2e-6 (the float32 rounding of O(1) sums of a few thousand terms) were chosen before measuring and kept; the
tightest comparison uses 93 % of its bound (avg_shortcut), the tightest of the pooling nets added later 60 % (avg_shortcut_v4).  All inputs and
seeds are fixed and the kernels deterministic, so the margins repeat run to run.
Value-only mutations of the engine (the interpreted chain launch's store, the max-pool VJP, one BatchNorm channel of the positive pass, each
scaled by 1 + 2^-10) each fail this file; the max-pool one passes the rest of the GPU suite.  So do these, tried once on lane 3 of the float4
kernels the backbones run (scaled by 1 + 2^-10 unless said otherwise), with the test that caught each:
  maxpool_bwd_kernel_v4<3,2>                 test_every_firing / test_schedule_matrix [stem_rows], [ceil_rows] (e_eng 5e-4 .. 1e-3)
  pool2_fwd_kernel's sum                     test_every_firing [mfm_pool2] P[0], test_pool_pair_fused_equals_separate_bits [mfm_pool2]
  ew_pool2_route in the float4 chain head    test_every_firing [mfm_pool2] P[3], test_pool_pair_fused_equals_separate_bits [mfm_pool2]
  avgpool_fwd_kernel_v4<2,2>                 test_every_firing / test_schedule_matrix [avg_shortcut_v4]
  normalize_bwd_kernel                       test_every_firing [encode_tail] P[2] (9e-5; [global_big], which has no normalize, passes)
  avgpool_global_bwd_kernel                  test_every_firing / test_schedule_matrix [global_big], [encode_tail]
  maxpool_fwd_kernel_rows<3,1>, the missing left column as a zero candidate instead of `continue`
                                             test_maxpool_forward_signed_and_special_values [stem_rows] (0 where -32 is due); no post-ReLU net can see it
  avgpool_global_fwd_kernel without its relu_in clamp (the fmaxf dropped)
                                             test_every_firing / test_schedule_matrix [signed_tail] (e_eng 1 .. 2; [encode_tail], which pools a post-ReLU map, passes)
XFR_LAYER_PARITY_REPORT=<path> writes every measured (e_eng, e32) pair there as JSON.

The pooling and tail kernels (xfr_amd/csrc/elementwise.hip) choose a variant by shape and pointer alignment; layer_nets.REQUIRED_VARIANTS names, per
net, the variants its runs must launch, and the library's launch counters (xfr_elementwise_launch_stats) prove they did: a workspace layout that leaves a pointer unaligned,
or a changed shape rule, fails with the name of the variant that no longer ran instead of quietly testing the scalar kernel.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_nets as L
from oracle import ebp_oracle as O
from parity_harness import FUSION_SEPARATE, MODES, Harness
from parity_utils import assert_map_close
from xfr_amd import _lib
from xfr_amd.engine import Engine

pytestmark = pytest.mark.gpu

h = Harness(switches=('lean', 'split', 'fusion', 'tail'))
_engine, _seed, _check, _apply = h.engine, h.seed, h.check, h.apply


@pytest.fixture(scope='module', autouse=True)
def _engines_and_report():
    yield
    h.finish('XFR_LAYER_PARITY_REPORT', merge=False)


def _assert_ran(name, where, before):
    after = _lib.elementwise_launch_stats()
    missing = [v for v in L.required_variants(name, where) if after[v] - before[v] <= 0]
    assert not missing, '%s/%s: no launch of %s (ran: %s)' % (name, where, ', '.join(missing), ', '.join(sorted(v for v in after if after[v] > before[v])))


def _oracle(case, x, seed, mode):
    """(P fp32 list, P fp64 list) of a sweep of the images x seeded with seed (N x D), after checking no max-pool window is a near-tie."""
    P64, _, tape64 = case.oracle_P(x, seed, mode, torch.float64)
    assert L.pool_windows_clear(tape64) == [], case.name
    P32, _, _ = case.oracle_P(x, seed, mode)
    return P32, P64


@pytest.mark.parametrize('name', [c.name for c in L.CASES])
def test_every_firing_matches_float64(gpu_device, name):
    """Engine.ebp_firing(k) -- the observed (literal) sweep -- for every firing k including k == firing_count (the P[-1] gather through the
    first layer), four subtree modes, one and three images, against the float64 tape's P[k]."""
    case = L.BY_NAME[name]
    eng = _engine(case, gpu_device)
    prog = case.program()
    st = prog.marks['classify']
    d = int(np.prod(eng.tensor_shape(st)))
    bad = []
    ran0 = _lib.elementwise_launch_stats()
    for n in (1, 3):
        x = case.inputs(n)
        seed = _seed(case, 1, n, d)
        for mode in MODES:
            eng.set_mode(mode)
            P32, P64 = _oracle(case, x, seed[0], mode)
            nf = eng.firing_count(st)
            assert nf + 1 == len(P64), (name, nf, len(P64))
            xd = x.to(gpu_device)
            for k in range(nf + 1):
                got = eng.ebp_firing(xd, st, seed.to(gpu_device), k)
                _check(bad, '%s/%s/n%d/P[%d]' % (name, mode, n, k), got, P32[k], P64[k])
    assert not bad, '\n'.join(bad)
    _assert_ran(name, 'firing', ran0)


# the schedule matrix: (tag, batch, streams, switches); the switches are reset to the engine's defaults after each entry
SCHEDULES = [
    ('default', 3, 1, {}),
    ('lean_b4', 4, 1, {'lean': 1}), ('lean_b8', 8, 1, {'lean': 1}), ('literal_b4', 4, 1, {'lean': 0}),
    ('split0', 3, 1, {'split': 0}), ('split3', 3, 1, {'split': 3}), ('split7', 3, 1, {'split': 7}), ('split7_lean_b4', 4, 1, {'split': 7}),
    ('fusion0', 3, 1, {'fusion': 0}), ('fusion7', 3, 1, {'fusion': 7}), ('fusion_separate', 3, 1, {'fusion': FUSION_SEPARATE}),
    ('tail_off', 3, 1, {'tail': 0}), ('tail_off_lean_b4', 4, 1, {'tail': 0}),
    ('streams2', 3, 2, {}), ('streams2_lean_b4', 4, 2, {}),
]
# one subtree mode per net (all four across the catalogue)
SCHEDULE_MODE = {'stem': 'affineonly_with_prior', 'projection': 'norelu', 'avg_shortcut': 'all', 'bf16x6': 'affineonly_with_prior',
                 'halo64': 'affineonly', 'halo65': 'all', 'mfm': 'affineonly', 'classifier': 'norelu', 'valid_wide': 'affineonly_with_prior',
                 'strided': 'all', 'stem_rows': 'norelu', 'ceil_rows': 'all', 'pool_generic': 'affineonly', 'pool_odd17': 'affineonly_with_prior',
                 'mfm_pool2': 'norelu', 'avg_shortcut_v4': 'affineonly', 'encode_tail': 'all', 'global_big': 'affineonly_with_prior',
                 'avg_generic': 'norelu', 'signed_tail': 'affineonly'}
NO_LEAN_NETS = ('mfm', 'classifier', 'mfm_pool2', 'encode_tail', 'global_big', 'signed_tail')
SPLIT_NETS = ('bf16x6', 'halo64', 'halo65')


@pytest.mark.parametrize('name', [c.name for c in L.CASES])
def test_schedule_matrix_pooled_matches_float64(gpu_device, name):
    """Engine.ebp(want_pooled=True), i.e. the un-observed sweep with every engine switch, against the float64 pooled P[-2]: lean at four and
    eight images and off, bf16x6 modes 0 / 3 / 7, epilogue fusion 0 / 3 / 7 (interpreted chains) / 3 with its bits 3, 4, 6, 7, 8 off, tail
    balancing on and off, two-stream sweeps (each stream's pooled MWP on its own).  The launch counters prove the lean and bf16x6 launches ran, and
    (layer_nets.REQUIRED_VARIANTS) that the fused and the separate forms of the pooling kernels ran where the switches ask for them."""
    case = L.BY_NAME[name]
    mode = SCHEDULE_MODE[name]
    eng = _engine(case, gpu_device)
    eng.set_mode(mode)
    prog = case.program()
    st = prog.marks['classify']
    d = int(np.prod(eng.tensor_shape(st)))
    lean_expected = name not in NO_LEAN_NETS
    cache = {}
    bad = []
    try:
        for tag, n, S, sw in SCHEDULES:
            if (n, S) not in cache:
                x = case.inputs(n, seed=1)
                seed = _seed(case, S, n, d, salt=1)
                refs = []
                for s in range(S):
                    P32, P64 = _oracle(case, x, seed[s], mode)
                    refs.append((P32[-2].sum(dim=1), P64[-2].sum(dim=1)))
                cache[(n, S)] = (x, seed, refs)
            x, seed, refs = cache[(n, S)]
            _apply(eng, sw)
            lean0, split0, ran0 = eng.lean_launches(), eng.split_gemm_launches(), _lib.elementwise_launch_stats()
            _, pooled = eng.ebp(x.to(gpu_device), st, seed.to(gpu_device), want_mwp=False, want_pooled=True)
            torch.cuda.synchronize()
            dl, ds = eng.lean_launches() - lean0, eng.split_gemm_launches() - split0
            for s in range(S):
                _check(bad, '%s/%s/%s/stream%d' % (name, mode, tag, s), pooled[s], refs[s][0], refs[s][1])
            _assert_ran(name, tag, ran0)
            if sw.get('lean', 1) and sw.get('fusion', 3) == 3 and n % 4 == 0:
                assert (dl > 0) == lean_expected, (name, tag, dl)
            elif n % 4 != 0 or not sw.get('lean', 1):
                assert dl == 0, (name, tag, dl)
            if name in SPLIT_NETS and sw.get('split') == 7:
                assert ds > 0, (name, tag, 'the bf16x6 kernel did not run')
            if sw.get('split') == 0 or (name in SPLIT_NETS and sw.get('split') == 3):
                assert ds == 0, (name, tag, ds)            # 0: off; 3: the grids of these nets stay below the 128 tiles the default asks for
    finally:
        _apply(eng, {})
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name', ['mfm_pool2', 'avg_shortcut_v4'])
def test_pool_pair_fused_equals_separate_bits(gpu_device, name):
    """pool2_fwd_kernel and ew_pool2_route (and the EW_AVGUP_IN head) promise the bits of the separate kernels: the pooled P[-2] with the default
    fusion and with fusion 0 is the same tensor, bit for bit (mode affineonly, three images) -- and so is every firing's own tensor (ebp_firing), the
    pools' among them, where no sum over channels could hide a pair of compensating differences."""
    case = L.BY_NAME[name]
    eng = _engine(case, gpu_device)
    eng.set_mode('affineonly')
    st = case.program().marks['classify']
    d = int(np.prod(eng.tensor_shape(st)))
    x = case.inputs(3, seed=4).to(gpu_device)
    seed = _seed(case, 1, 3, d, salt=4).to(gpu_device)
    nf = eng.firing_count(st)
    firing_names = eng.firing_names(st) + ['image']
    got, fired = {}, {}
    try:
        for tag, fusion in (('default', 3), ('fusion0', 0)):
            _apply(eng, {'fusion': fusion})
            ran0 = _lib.elementwise_launch_stats()
            _, pooled = eng.ebp(x, st, seed, want_mwp=False, want_pooled=True)
            got[tag] = pooled.cpu()
            _assert_ran(name, tag, ran0)
            ran0 = _lib.elementwise_launch_stats()
            fired[tag] = [eng.ebp_firing(x, st, seed, k).cpu() for k in range(nf + 1)]
            _assert_ran(name, tag, ran0)
    finally:
        _apply(eng, {})
    a, b = got['default'], got['fusion0']
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    diff = (a.double() - b.double()).abs()
    assert torch.equal(a, b), '%s: fused and separate pooled P[-2] differ in %d of %d elements, max |d| %.3e (max |P| %.3e)' % (
        name, int((a != b).sum()), a.numel(), float(diff.max()), float(a.abs().max()))
    assert any('Pool' in n for n in firing_names), firing_names
    bad = ['P[%d] (%s): %d of %d elements, max |d| %.3e (max |P| %.3e)' % (k, firing_names[k], int((u != v).sum()), u.numel(),
                                                                          float((u.double() - v.double()).abs().max()), float(u.abs().max()))
           for k, (u, v) in enumerate(zip(fired['default'], fired['fusion0'])) if not torch.equal(u, v)]
    assert not bad, '%s: fused and separate firings differ:\n%s' % (name, '\n'.join(bad))


# the pooled maps of test_maxpool_forward_signed_and_special_values: (name, C x H x W of the pool's input, kernel, stride, pad, ceil_mode, variant)
SIGNED_POOLS = [
    ('stem_rows', (8, 13, 16), 3, 2, 1, False, 'maxpool_fwd_rows<3,1>'),
    ('ceil_rows', (8, 12, 16), 3, 2, 0, True, 'maxpool_fwd_rows<3,0>'),
    ('pool_generic', (8, 12, 12), 3, 3, 0, False, 'maxpool_fwd_v4<0,0>'),
    ('pool_odd17', (8, 10, 17), 2, 2, 0, False, 'maxpool_fwd_v4<2,2>'),
]


def _signed_pool_case(shape, k, stride, pad, ceil_mode, kind):
    """conv 1x1 -> Multiply(2) -> conv 1x1 with bias -> max-pool -> Linear: the pool reads a signed map (no BatchNorm / ReLU in front of it; the
    first two layers are there because the planner ends a sweep at the first layer's output and walks to it through an elementwise op).
    kind 'negative': random weights and a bias of -40, every value of the map is negative (a pool that pads with 0 instead of -inf returns 0 at the
    edges); 'ties': identity weights, bias 0.5 and inputs from {-3 .. 3}, so the map holds exact ties in almost every window and is the same
    in float32 and float64."""
    c, h, w = shape
    pooled = tuple(F.max_pool2d(torch.zeros((1, 1, h, w)), k, stride, pad, 1, ceil_mode).shape[2:])
    marks = {}

    def fwd(p):
        marks['conv'] = p.conv(p.multiply(p.conv(0, 'conv0', c, 1, bias=False), 2.0), 'conv1', c, 1, bias=True)
        marks['pool'] = p.maxpool(marks['conv'], k, stride, pad, ceil_mode=ceil_mode)
        return p.mark('classify', p.linear(marks['pool'], 'fc', 5, pooled))
    case = L.NetCase('signed_%s' % kind, shape, fwd, 'max-pool of a signed map', 23)
    g = torch.Generator().manual_seed(29 + c * h * w)
    fc = torch.randn((5, c * pooled[0] * pooled[1]), generator=g) / np.sqrt(c * pooled[0] * pooled[1])
    if kind == 'negative':
        w0, wt, b = torch.randn((c, c, 1, 1), generator=g) / np.sqrt(c), torch.randn((c, c, 1, 1), generator=g) / np.sqrt(c), torch.full((c,), -40.0)
    else:
        w0, wt, b = torch.eye(c).reshape(c, c, 1, 1).clone(), torch.eye(c).reshape(c, c, 1, 1).clone(), torch.full((c,), 0.5)
    case._params = {'conv0.weight': w0, 'conv1.weight': wt, 'conv1.bias': b, 'fc.weight': fc, 'fc.bias': torch.zeros((5,))}
    case.program()
    return case, dict(marks)


@pytest.mark.parametrize('pool', SIGNED_POOLS, ids=[p[0] for p in SIGNED_POOLS])
def test_maxpool_forward_signed_and_special_values(gpu_device, pool):
    """The max-pool kernels on signed maps, which no network of the suite gives them (every pooled map there is post-ReLU): padding is -inf, not 0,
    and among equal values the first in (kh, kw) order wins.  Engine.forward of the pool's output equals float32 F.max_pool2d of the engine's own
    convolution output bit for bit, on an all-negative map and on a map with exact ties planted; on the latter every firing of one sweep in mode
    norelu (the max-pool VJP follows the argmax bytes) meets the float64 rule."""
    name, shape, k, stride, pad, ceil_mode, variant = pool
    n = 3
    for kind in ('negative', 'ties'):
        case, marks = _signed_pool_case(shape, k, stride, pad, ceil_mode, kind)
        g = torch.Generator().manual_seed(37)
        x = torch.randn((n,) + shape, generator=g) if kind == 'negative' else torch.randint(-3, 4, (n,) + shape, generator=g).float()
        eng = Engine(case.program(), n, gpu_device)
        try:
            eng.load_weights(case.params())
            ran0 = _lib.elementwise_launch_stats()
            conv = eng.forward(x.to(gpu_device), marks['conv']).cpu()
            got = eng.forward(x.to(gpu_device), marks['pool']).cpu()
            ran = _lib.elementwise_launch_stats()
            assert ran[variant] > ran0[variant], '%s/%s: no launch of %s' % (name, kind, variant)
            want = F.max_pool2d(conv, k, stride, pad, 1, ceil_mode)
            assert got.shape == want.shape and bool(torch.isfinite(got).all())
            if kind == 'negative':
                assert float(conv.max()) < 0 and float(got.max()) < 0, (name, float(conv.max()), float(got.max()))
            else:
                tape64, _ = case.tape(x, torch.float64)
                assert torch.equal(conv.double(), tape64.T[marks['conv']]), name           # the map is exact in both precisions
                top2 = L.pool_window_columns(conv, k, stride, pad, want.shape[2:]).topk(2, dim=2).values
                assert float((top2[:, :, 0] == top2[:, :, 1]).float().mean()) > 0.2, name      # ties planted in many windows
            assert torch.equal(got, want), '%s/%s: %d of %d pooled values differ from F.max_pool2d, max |d| %.3e' % (
                name, kind, int((got != want).sum()), got.numel(), float((got - want).abs().max()))
            if kind == 'ties':
                eng.set_mode('norelu')
                st = case.program().marks['classify']
                d = int(np.prod(eng.tensor_shape(st)))
                seed = _seed(case, 1, n, d, salt=5)
                P64, _, t64 = case.oracle_P(x, seed[0], 'norelu', torch.float64)
                P32, _, _ = case.oracle_P(x, seed[0], 'norelu')
                assert L.pool_windows_clear(t64) == []                                     # exact ties only: the first-index rule decides them
                nf = eng.firing_count(st)
                assert nf + 1 == len(P64)
                bad = []
                for kf in range(nf + 1):
                    _check(bad, 'signed/%s/norelu/P[%d]' % (name, kf), eng.ebp_firing(x.to(gpu_device), st, seed.to(gpu_device), kf), P32[kf], P64[kf])
                assert not bad, '\n'.join(bad)
        finally:
            eng.close()


def test_batch32_forward_split(gpu_device):
    """One batch of 32 images (the forward-only split into two half batches on the internal streams, on and off): the encoding and the pooled
    P[-2] of a projection block net against float64."""
    case = L.BY_NAME['projection']
    mode = 'affineonly_with_prior'
    eng = _engine(case, gpu_device, max_batch=32)
    eng.set_mode(mode)
    st = case.program().marks['classify']
    d = int(np.prod(eng.tensor_shape(st)))
    x = case.inputs(32, seed=2)
    seed = _seed(case, 1, 32, d, salt=2)
    P32, P64 = _oracle(case, x, seed[0], mode)
    tape64, out64 = case.tape(x, torch.float64)
    tape32, out32 = case.tape(x)
    bad = []
    try:
        for split in (1, 0):
            eng.set_forward_split(split)
            y = eng.forward(x.to(gpu_device), st)
            _check(bad, 'projection/b32/forward_split%d/classify' % split, y.reshape(32, -1), tape32.T[out32], tape64.T[out64])
            _, pooled = eng.ebp(x.to(gpu_device), st, seed.to(gpu_device))
            _check(bad, 'projection/b32/forward_split%d/pooled' % split, pooled[0], P32[-2].sum(dim=1), P64[-2].sum(dim=1))
    finally:
        eng.set_forward_split(1)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name', ['stem', 'avg_shortcut', 'mfm'])
def test_truncated_contrastive_tail_on_engine_P(gpu_device, name):
    """contrastive(..., percentile) equals whitebox.py:547-558 (sort, cumsum, percentile mask, relu of the masked difference, saliency) applied
    on the CPU to the engine's own P[-2] at the catalogue's shapes."""
    import torch.nn.functional as F
    case = L.BY_NAME[name]
    eng = _engine(case, gpu_device)
    eng.set_mode('affineonly_with_prior')
    st = case.program().marks['classify']
    d = int(np.prod(eng.tensor_shape(st)))
    n = 3
    x = case.inputs(n, seed=3).to(gpu_device)
    seeds = _seed(case, 2, n, d, salt=3).to(gpu_device)
    mwp, _ = eng.ebp(x, st, seeds, want_mwp=True)
    mwp = mwp.cpu()
    for pct in (20.0, 50.0, 0.0):
        sal = eng.contrastive(x, st, seeds, pct).cpu().numpy()
        for i in range(n):
            m = mwp[0, i:i + 1] / torch.sum(mwp[0, i:i + 1])
            q = mwp[1, i:i + 1] / torch.sum(mwp[1, i:i + 1])
            (s, idx) = torch.sort(torch.flatten(m.clone()))
            cs = torch.cumsum(s, 0)
            mask = torch.zeros(s.shape)
            mask[idx] = (cs >= (pct / 100.0) * cs[-1]).type(torch.FloatTensor)
            mask = mask.reshape(m.shape)
            c = np.squeeze(np.sum(F.relu(mask * m - mask * q).numpy(), axis=1).astype(np.float32))
            assert_map_close(sal[i], O.mwp_to_saliency(c), '%s truncated tail pct=%g sample %d' % (name, pct, i))


@pytest.mark.parametrize('hw', [(1, 1), (2, 5), (7, 7), (113, 111)])
def test_saliency_of_several_maps_in_one_call(gpu_device, hw):
    """mwp_to_saliency on three maps in one call, the middle one all zero (the max(sum, eps) guard), against the scipy oracle map by map."""
    eng = _engine(L.BY_NAME['mfm'], gpu_device, max_batch=32)
    rng = np.random.RandomState(hw[0] * 1000 + hw[1])
    P = (rng.rand(3, *hw) ** 4).astype(np.float32)
    P[1] = 0.0
    got = eng.mwp_to_saliency(torch.as_tensor(P).to(gpu_device)).cpu().numpy()
    assert got.shape == P.shape and np.isfinite(got).all()
    for i in range(3):
        want = O.mwp_to_saliency(P[i])
        if i == 1:
            assert np.all(got[i] == 0)
        else:
            assert np.abs(got[i] - want).max() <= 2e-7 * want.max(), (hw, i)
            assert abs(float(got[i].sum()) - 1.0) < 1e-5


@pytest.mark.parametrize('shape', [
    # cin, h, w, nb, cout, k, stride, pad  (the table of test_gpu_parity.test_conv_gemm_matches_fp32_reference)
    (3, 32, 32, 3, 64, 7, 2, 3), (1, 20, 20, 2, 96, 5, 1, 2), (64, 14, 14, 5, 64, 3, 1, 1), (48, 9, 9, 3, 96, 3, 1, 1),
    (256, 7, 7, 2, 130, 1, 1, 0), (128, 8, 8, 4, 256, 1, 1, 0), (64, 16, 16, 2, 32, 1, 2, 0), (128, 8, 8, 2, 40, 8, 1, 0),
    (256, 14, 14, 5, 256, 3, 1, 1), (1024, 14, 14, 3, 128, 1, 1, 0), (8192, 1, 1, 2, 256, 1, 1, 0), (256, 1, 1, 1, 1037, 1, 1, 0),
])
@pytest.mark.parametrize('cfg', [0, 9, 30005])
def test_conv_gemm_relu_in_matches_float64(gpu_device, shape, cfg):
    """xfr_debug_conv with relu_in = 1 (the GEMM applies ReLU to its operand as it stages it) against float64 conv2d(relu(x)); the inputs are
    centred, so half the operand is clipped."""
    lib = _lib.load()
    cin, h, w, nb, cout, k, stride, pad = shape
    g = torch.Generator().manual_seed(4)
    x = torch.randn((nb, cin, h, w), generator=g)
    wt = torch.randn((cout, cin, k, k), generator=g) / np.sqrt(cin * k * k)
    b = torch.randn((cout,), generator=g)
    want = torch.nn.functional.conv2d(torch.relu(x).double(), wt.double(), b.double(), stride=stride, padding=pad)
    want32 = torch.nn.functional.conv2d(torch.relu(x), wt, b, stride=stride, padding=pad)
    xg = x.to(gpu_device).permute(1, 0, 2, 3).contiguous()
    out = torch.full((cout, nb) + tuple(want.shape[2:]), float('nan'), device=gpu_device)
    ms = ctypes.c_float()
    _lib.check(lib.xfr_debug_conv(xg.data_ptr(), wt.data_ptr(), b.data_ptr(), out.data_ptr(), cin, h, w, nb, cout, k, k,
                                  stride, pad, 1, cfg, 1, ctypes.byref(ms)))
    got = out.permute(1, 0, 2, 3).cpu()
    bad = []
    _check(bad, 'debug_conv/relu_in/%s/cfg%d' % ('x'.join(str(v) for v in shape), cfg), got, want32, want)
    assert not bad, '\n'.join(bad)
