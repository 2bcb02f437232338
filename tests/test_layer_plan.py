"""The catalogue of small layer programs (tests/layer_nets.py), without a GPU: the planner routes every net to the launch form it exists for,
and the float64 oracle tape agrees with the float32 one on each of them (the yardstick of tests/test_gpu_layer_parity.py)."""
import os
import re

import pytest
import torch

import layer_nets as L
from oracle import ebp_oracle as O
from xfr_amd.program import OpKind

MODES = ('affineonly', 'affineonly_with_prior', 'norelu', 'all')


def _describe(case, mode='affineonly_with_prior', batch=4, fusion=None):
    prog = case.program()
    if fusion is not None:
        os.environ['XFR_DESCRIBE_FUSION'] = str(fusion)
    try:
        return prog.describe(mode, prog.marks['classify'], batch=batch)
    finally:
        os.environ.pop('XFR_DESCRIBE_FUSION', None)


def _bwd(text):
    return [ln for ln in text.splitlines() if ln.startswith('bwd ')]


def _lean_count(text):
    m = re.search(r'^lean convolutions (\d+)$', text, re.M)
    return int(m.group(1)) if m else 0


def _has(lines, pattern):
    return any(re.search(pattern, ln) for ln in lines)


# what each net's sweep must contain (regular expressions over the `bwd` lines of the default schedule) and its count of lean convolutions
EXPECT = {
    'stem': ([r'^bwd CONV_BWD src \d+ dst \d+ acc 0 \[40 x 10 x 8\] K 400 SIG .* compiled=\d+$',
              r'^bwd CONV_BWD .* \[64 x 10 x 8\] K 360 SIG',
              r'^bwd MAXPOOL_BWD .* \[64 x 19 x 15\]$', r'^bwd EW src \d+ dst 1 '], 1),
    'projection': ([r'^bwd ZERO src -1 dst 3 .* \[64 x 15 x 13\]$',
                    r'^bwd CONV_BWD src 12 dst 3 acc 1 \[64 x 15 x 13\] K 128$',               # the projection's stride-2 scatter, accumulating
                    r'^bwd CONV_BWD src 4 dst 3 acc 1 \[64 x 15 x 13\] K 32$',                 # the main path's stride-2 scatter
                    r'^bwd CONV_BWD src 16 dst 12 .* SIG .* compiled=-1$'], 4),                # the Linear head + block chain: interpreted
    'avg_shortcut': ([r'^bwd CONV_BWD src 4 dst 3 acc 0 \[64 x 18 x 14\] K 32$',
                      r'^bwd EW src 13 dst 1 acc 0 \[64 x 18 x 14\] steps 7$'], 3),            # the EW_AVGUP_IN head of the block-input chain
    'bf16x6': ([r'^bwd CONV_BWD src 7 dst 4 acc 0 \[128 x 15 x 17\] K 1152 SIG .* compiled=\d+$',
                r'^bwd CONV_BWD src 4 dst 1 acc 0 \[128 x 15 x 17\] K 1152 SIG',
                r'^bwd CONV_BWD src 11 dst 7 acc 0 \[128 x 15 x 17\] K 256 SIG'], 4),
    'halo64': ([r'^bwd CONV_BWD src 4 dst 1 acc 0 \[128 x 9 x 63\] K 1152 SIG'], 1),
    'halo65': ([r'^bwd CONV_BWD src 4 dst 1 acc 0 \[128 x 9 x 64\] K 1152 SIG'], 1),
    'mfm': ([r'^bwd CONV_BWD src 10 dst 9 acc 0 \[8 x 18 x 15\] K 1350 SIG 0701 compiled=\d+$',
             r'^bwd CONV_BWD src 7 dst 6 acc 0 \[8 x 18 x 15\] K 144 SIG',
             r'^bwd AVGPOOL_BWD src 6 dst 3 acc 0 \[8 x 37 x 31\]$', r'^bwd MAXPOOL_BWD src 6 dst 3 acc 1 \[8 x 37 x 31\]$'], 0),
    'classifier': ([r'^bwd CONV_BWD src 4 dst 1 acc 0 \[512 x 4 x 5\] K 20740 SIG'], 0),
    'valid_wide': ([r'^bwd CONV_BWD src 10 dst 7 acc 0 \[16 x 9 x 9\] K 405 SIG',
                    r'^bwd CONV_BWD src 7 dst 4 acc 0 \[32 x 7 x 7\] K 144 SIG',             # 3x3 pad 2: backward padding 0
                    r'^bwd CONV_BWD src 4 dst 1 acc 0 \[24 x 11 x 11\] K 800 SIG'], 1),       # 'valid' 5x5: backward padding 4; Cin 24: no lean form
    'strided': ([r'^bwd ZERO src -1 dst 3 .* \[32 x 10 x 7\]$', r'^bwd CONV_BWD src 4 dst 3 acc 1 \[32 x 10 x 7\] K 48$'], 1),
    'stem_rows': ([r'^bwd MAXPOOL_BWD .* \[64 x 13 x 16\]$'], 1),
    'ceil_rows': ([r'^bwd MAXPOOL_BWD .* \[64 x 12 x 16\]$'], 1),
    'pool_generic': ([r'^bwd MAXPOOL_BWD .* \[32 x 12 x 12\]$'], 1),
    'pool_odd17': ([r'^bwd MAXPOOL_BWD .* \[32 x 10 x 17\]$'], 1),
    'mfm_pool2': ([r'^bwd EW src 6 dst 1 acc 0 \[8 x 20 x 24\] steps 5$'], 0),                  # the EW_POOL2_IN head: no separate pool VJPs (below)
    'avg_shortcut_v4': ([r'^bwd EW src 13 dst 1 acc 0 \[64 x 16 x 24\] steps 7$'], 3),
    'encode_tail': ([r'^bwd NORMALIZE_BWD src 5 dst 4 acc 0 \[80 x 1 x 1\]$', r'^bwd AVGPOOL_BWD src 4 dst 3 acc 0 \[80 x 5 x 5\]$'], 0),
    'global_big': ([r'^bwd AVGPOOL_BWD src 4 dst 3 acc 0 \[48 x 12 x 12\]$'], 0),
    'avg_generic': ([r'^bwd AVGPOOL_BWD .* \[32 x 12 x 12\]$'], 1),
    'signed_tail': ([r'^bwd CONV_BWD src 4 dst 3 acc 0 \[80 x 1 x 1\] K 5 SIG',                 # the Linear head divides by the pool's positive value
                     r'^bwd AVGPOOL_BWD src 3 dst 2 acc 0 \[80 x 5 x 5\]$'], 0),
}


def test_catalogue_covers_every_case():
    assert sorted(EXPECT) == sorted(L.BY_NAME)


@pytest.mark.parametrize('name', sorted(L.BY_NAME))
def test_plan_routes_the_net_to_its_launch_form(name):
    """prog.describe shows the launch form the net exists for, in every subtree mode; the firing order is the oracle's; a later planner change
    that routes a net elsewhere fails here instead of quietly testing something else."""
    case = L.BY_NAME[name]
    patterns, lean = EXPECT[name]
    prog = case.program()
    x = case.inputs(1)
    for mode in MODES:
        text = _describe(case, mode)
        lines = _bwd(text)
        for pat in patterns:
            if mode in ('norelu', 'all') and 'SIG' in pat:
                pat = pat.split(' SIG')[0]          # the chains differ by mode; the GEMMs do not
            assert _has(lines, pat), '%s/%s: no launch matches %r\n%s' % (name, mode, pat, text)
        assert _lean_count(text) == lean, '%s/%s\n%s' % (name, mode, text)
        # firing order = the reference's (the oracle tape's hook order, image hook last)
        ops = prog.firing_ops(mode, prog.marks['classify'])
        tape, out = case.tape(x)
        _, names, _ = case.oracle_P(x, torch.ones(tape.T[out].shape), mode)
        kinds = [OpKind(prog.ops[k].kind) for k in ops]
        want = [{'Conv2d': OpKind.CONV, 'BatchNorm2d': OpKind.BATCHNORM, 'ReLU': OpKind.RELU, 'MaxPool2d': OpKind.MAXPOOL,
                 'AvgPool2d': OpKind.AVGPOOL, 'Add': OpKind.ADD, 'ConcatChannels': OpKind.CONCAT, 'Linear': OpKind.LINEAR,
                 'Split': OpKind.SPLIT, 'Multiply': OpKind.MULTIPLY}[n] for n in names[:-1]]
        assert kinds == want, (name, mode)


def test_fusion_switches_change_the_launch_forms():
    """The fusion bits the GPU schedule matrix turns off really move those nets to the separate launches."""
    avg = L.BY_NAME['avg_shortcut']
    kinds = [ln.split()[1] for ln in _bwd(_describe(avg, fusion=67))]
    assert 'AVGPOOL_BWD' in kinds and 'COPY' in kinds, kinds                   # bit 6 off: no EW_AVGUP_IN head
    assert 'AVGPOOL_BWD' not in [ln.split()[1] for ln in _bwd(_describe(avg))]
    proj = L.BY_NAME['projection']
    n_default = len(_bwd(_describe(proj)))
    assert len(_bwd(_describe(proj, fusion=131))) > n_default                 # bit 7 off: the main path's chain as its own launch
    assert len(_bwd(_describe(proj, fusion=0))) > n_default                   # everything un-fused
    # the pool pair: one chain launch with the EW_POOL2_IN head by default, its two VJPs at fusion 0 -- and always at odd sizes (`mfm`)
    pool_vjps = lambda text: sorted(k for k in (ln.split()[1] for ln in _bwd(text)) if k in ('AVGPOOL_BWD', 'MAXPOOL_BWD'))
    pair = L.BY_NAME['mfm_pool2']
    assert pool_vjps(_describe(pair)) == []
    assert pool_vjps(_describe(pair, fusion=0)) == ['AVGPOOL_BWD', 'MAXPOOL_BWD']
    assert pool_vjps(_describe(L.BY_NAME['mfm'])) == ['AVGPOOL_BWD', 'MAXPOOL_BWD']
    # a global pool keeps its VJP launch under both settings
    for fusion in (None, 0):
        assert _has(_bwd(_describe(L.BY_NAME['global_big'], fusion=fusion)), r'^bwd AVGPOOL_BWD src 4 dst 3 acc 0 \[48 x 12 x 12\]$')


def test_required_variants_cover_every_pool_normalize_and_stem_kernel():
    """layer_nets.REQUIRED_VARIANTS (what tests/test_gpu_layer_parity.py proves with the launch counters) names every pooling, normalize and direct-stem
    variant the library can launch, and nothing it cannot: a variant added later cannot go without a float64 comparison silently."""
    from xfr_amd import _lib
    names = _lib.elementwise_variant_names()
    assert len(names) == len(set(names)) and _lib.load().xfr_elementwise_variant_name(len(names)) is None
    required = set(v for by_where in L.REQUIRED_VARIANTS.values() for vs in by_where.values() for v in vs)
    assert required <= set(names), required - set(names)
    assert set(L.REQUIRED_VARIANTS) <= set(L.BY_NAME)
    kernels = set(n for n in names if not n.startswith('ew_chain'))
    assert set(v for v in required if not v.startswith('ew_chain')) == kernels, kernels - required
    assert set(v for v in required if v.startswith('ew_chain')) == {'ew_chain_v4/pool2_in', 'ew_chain_v4/avgup_in'}


def test_signed_tail_pools_a_signed_map():
    """`signed_tail` exists for the clamp in the positive pass of the global average pool (the engine sets relu_in where the pooled map is not provably
    >= 0): its pooled map has values of both signs in every image, so avg(relu(x)) -- the x the Linear head divides by -- is far from avg(x)."""
    case = L.BY_NAME['signed_tail']
    tape64, _ = case.tape(case.inputs(3), torch.float64)
    pool = [c for c in tape64.calls if c.name == 'AvgPool2d']
    assert len(pool) == 1 and not any(c.name == 'ReLU' for c in tape64.calls)
    v = tape64.T[pool[0].ins[0]]
    assert tuple(v.shape[1:]) == (80, 5, 5)
    neg = (v < 0).double().mean(dim=(1, 2, 3))
    assert float(neg.min()) > 0.25 and float(neg.max()) < 0.75, neg
    clamped, plain = torch.relu(v).mean(dim=(2, 3)), v.mean(dim=(2, 3))
    assert float((clamped - plain).abs().max()) > 0.1 * float(clamped.abs().max())


@pytest.mark.parametrize('name', sorted(L.BY_NAME))
def test_float64_tape_agrees_with_float32(name):
    """The yardstick itself: on every net and mode the float64 tape's P list equals the float32 tape's to float32 rounding (and both see the
    same argmax in every max-pool / MaxFeatureMap window, by a margin)."""
    case = L.BY_NAME[name]
    x = case.inputs(3)
    tape64, out = case.tape(x, torch.float64)
    assert tape64.T[out].dtype == torch.float64
    assert L.pool_windows_clear(tape64) == []
    seed = torch.rand(tape64.T[out].shape, generator=torch.Generator().manual_seed(5))
    for mode in MODES:
        P64, names64, _ = case.oracle_P(x, seed, mode, torch.float64)
        P32, names32, _ = case.oracle_P(x, seed, mode)
        assert names64 == names32 and len(P64) == len(P32)
        for k, (a, b) in enumerate(zip(P32, P64)):
            assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == b.shape
            scale = float(b.abs().max())
            assert scale > 0, (name, mode, k)
            assert float((a.double() - b).abs().max()) <= 1e-5 * scale, (name, mode, k)


def test_float32_tape_is_the_default():
    """Tape(dtype=float32) is the tape as it was: the parameters dict is used as given (no copy), values stay float32."""
    case = L.BY_NAME['strided']
    sd = case.params()
    tape = O.Tape(sd)
    assert tape.p is sd and tape.dtype == torch.float32
    t64 = O.Tape(sd, dtype=torch.float64)
    assert all(v.dtype == torch.float64 for v in t64.p.values())
