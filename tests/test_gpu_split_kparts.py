"""K-parts of the bf16x6 GEMM kernel (conv_gemm_split.hip): a tile's K range cut into S parts on S workgroups, met in the tail workspace.

Through xfr_debug_conv with configuration 9 and the part count forced (cfg = 9 + 10000 * S), at the smallest shapes where each piece can go
wrong: 7 x 7 maps of 3 images (M = 147: two m-tiles, the second a tail, tiles spanning image borders);
  patch mode (3x3 pad 1, Cout 128):  Cin 32, S 2 -- one channel block per part, the second part starts negated;  Cin 48, S 2 -- parts of 2 + 1 blocks;
  slab mode (1x1, Cout 256):  Cin 96, S 2 -- one pass per part, the second starts negated;  Cin 80, S 2 -- five K-steps, the last pass short;
                              Cin 144, S 3.
Yardstick: float64 conv2d on the CPU and the rule of tests/test_gpu_layer_parity.py, e_eng <= max(4 e32, 2e-6) with e32 the fp32 CPU result's
own error -- the bound comes from the reference computation.  The engine leg runs the `bf16x6` net of tests/layer_nets.py (dual W / relu(W)
launches, compiled chain epilogues, fp32 tail-balanced launches on the same stream and workspace) in a child process whose environment opens
the host rule (read once per process) to three parts on these maps, and reads the part count of every launch from the launch log.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

if __name__ == '__main__':       # the engine leg's child process (below): the paths pytest's conftest gives the suite
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]

import numpy as np
import pytest
import torch

import layer_nets as L
from parity_harness import FLOOR, K_RATIO
from xfr_amd import _lib
from xfr_amd.engine import Engine

pytestmark = pytest.mark.gpu

# cin, k, pad, cout, S
PATCH = [(32, 3, 1, 128, 2), (48, 3, 1, 128, 2)]
SLAB = [(96, 1, 0, 256, 2), (80, 1, 0, 256, 2), (144, 1, 0, 256, 3)]
CASES = PATCH + SLAB
H = W = 7
NB = 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'split_kparts_cfg9_bits.json')
_REF = {}


def case_id(c):
    return 'cin%d_k%d_cout%d_S%d' % (c[0], c[1], c[3], c[4])


def shape_id(c):
    return 'cin%d_k%d_cout%d' % (c[0], c[1], c[3])


def case_inputs(c, relu_in):
    """(x, w, b, fp32 reference, float64 reference) of a case, computed once."""
    key = (c[:4], relu_in)
    if key not in _REF:
        cin, k, pad, cout = c[:4]
        g = torch.Generator().manual_seed(1000 + cin + 7 * k)
        x = torch.randn((NB, cin, H, W), generator=g)
        wt = torch.randn((cout, cin, k, k), generator=g) / np.sqrt(cin * k * k)
        b = torch.randn((cout,), generator=g)
        xr = torch.relu(x) if relu_in else x
        want = torch.nn.functional.conv2d(xr.double(), wt.double(), b.double(), padding=pad)
        want32 = torch.nn.functional.conv2d(xr, wt, b, padding=pad)
        _REF[key] = (x, wt, b, want32, want)
    return _REF[key]


def run_conv(device, c, relu_in, cfg, reps=1):
    """One xfr_debug_conv call (reps warm-up launches + reps timed ones on one stream and one workspace); the output as [nb, cout, h, w] on the CPU."""
    cin, k, pad, cout = c[:4]
    x, wt, b, _, _ = case_inputs(c, relu_in)
    xg = x.to(device).permute(1, 0, 2, 3).contiguous()
    out = torch.full((cout, NB, H, W), float('nan'), device=device)
    ms = ctypes.c_float()
    _lib.check(_lib.load().xfr_debug_conv(xg.data_ptr(), wt.data_ptr(), b.data_ptr(), out.data_ptr(), cin, H, W, NB, cout, k, k, 1, pad,
                                          relu_in, cfg, reps, ctypes.byref(ms)))
    torch.cuda.synchronize()
    return out.permute(1, 0, 2, 3).cpu()


def rel(a, ref):
    return float((a.double() - ref).abs().max()) / float(ref.abs().max())


def check_rule(tag, got, want32, want):
    assert bool(torch.isfinite(got).all()), '%s: non-finite values' % tag
    e_eng, e32 = rel(got, want), rel(want32, want)
    print('%s: e_eng %.3e e32 %.3e' % (tag, e_eng, e32))
    assert e_eng <= max(K_RATIO * e32, FLOOR), '%s: e_eng %.3e > max(%g x e32 %.3e, %g)' % (tag, e_eng, K_RATIO, e32, FLOOR)


def bits(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize('relu_in', [0, 1])
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_forced_parts_match_float64_and_repeat(gpu_device, case, relu_in):
    """S forced parts against float64; the same forced launch again is bit-identical (the last arriver sums in part order, whoever it is)."""
    _, _, _, want32, want = case_inputs(case, relu_in)
    cfg = 9 + 10000 * case[4]
    got = run_conv(gpu_device, case, relu_in, cfg)
    check_rule('%s/relu_in%d' % (case_id(case), relu_in), got, want32, want)
    again = run_conv(gpu_device, case, relu_in, cfg)
    assert torch.equal(got, again), 'two launches with %d forced parts differ' % case[4]


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_every_part_count_matches_float64(gpu_device, case):
    """Every part count the units allow (patch: channel blocks, slab: passes of three K-steps), up to 4, and the host's own choice (cfg 9)."""
    cin, k = case[:2]
    units = cin // 16 if k == 3 else (cin // 16 + 2) // 3
    _, _, _, want32, want = case_inputs(case, 0)
    for S in [0] + list(range(2, min(units, 4) + 1)):
        got = run_conv(gpu_device, case, 0, 9 + 10000 * S)
        check_rule('%s/forced%d' % (case_id(case), S), got, want32, want)


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_one_part_keeps_the_unsplit_kernels_bits(gpu_device, case):
    """S = 1 forced is the launch without parts: bit for bit what configuration 9 gave before the kernel knew parts (tests/golden: SHA-256 of the
    output, recorded with the previous kernel on an MI355X for these inputs), for both input forms."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    for relu_in in (0, 1):
        got = run_conv(gpu_device, case, relu_in, 10009)
        _, _, _, want32, want = case_inputs(case, relu_in)
        check_rule('%s/one_part/relu_in%d' % (case_id(case), relu_in), got, want32, want)
        assert bits(got) == golden['%s/relu_in%d' % (shape_id(case), relu_in)], 'S = 1 moved the bits of the un-split launch'


def test_counters_return_to_zero_between_launches(gpu_device):
    """xfr_debug_conv keeps ONE tail workspace and ONE set of arrival counters for the whole process, zeroed when they are made and never again.
    So this sequence shares them like the launches of an engine stream: two parts (patch), three parts (slab), the fp32 kernel's tail-balanced
    K-parts, two parts again, three parts on the other shape -- different inputs, each into an output filled with NaN.  A launch that left
    its tile's counter behind (old value S instead of 0) would keep every later launch on that tile from ever seeing S - 1 arrivals: no part
    reduces, the NaNs stay.  Each call is two launches (warm-up + timed), so the second launch of a call depends on the first one's reset too."""
    seq = [(PATCH[1], 20009), (SLAB[2], 30009), (PATCH[1], 30005), (SLAB[2], 30005), (PATCH[0], 20009), (SLAB[2], 20009), (PATCH[1], 30009), (SLAB[0], 20009)]
    for rnd in range(2):
        for case, cfg in seq:
            _, _, _, want32, want = case_inputs(case, rnd)
            got = run_conv(gpu_device, case, rnd, cfg)
            check_rule('%s/cfg%d/round%d' % (case_id(case), cfg, rnd), got, want32, want)


ENGINE_LEG_ENV = {'XFR_SPLIT_PARTS_BELOW_HW': '1000000', 'XFR_SPLIT_MAX_PARTS': '3', 'XFR_SPLIT_MIN_CB': '2', 'XFR_SPLIT_MIN_STEPS': '6'}


def engine_leg():
    """Child process: the `bf16x6` net with the bf16x6 kernel on every grid, the launch log on; prints one JSON object."""
    from xfr_amd import tuning
    dev = torch.device('cuda', 0)
    case = L.BY_NAME['bf16x6']
    mode = 'affineonly_with_prior'
    eng = Engine(case.program(), 8, dev)
    out = {'runs': [], 'launches': []}
    try:
        eng.load_weights(case.params())
        eng.set_mode(mode)
        st = case.program().marks['classify']
        d = int(np.prod(eng.tensor_shape(st)))
        eng.set_split_gemm(7)
        for n in (3, 4):
            x = case.inputs(n, seed=1)
            g = torch.Generator().manual_seed(97 + n)
            seed = torch.rand((1, n, d), generator=g)
            P64, _, _ = case.oracle_P(x, seed[0], mode, torch.float64)
            P32, _, _ = case.oracle_P(x, seed[0], mode)
            want32, want = P32[-2].sum(dim=1), P64[-2].sum(dim=1)
            runs = []

            def step():
                _, pooled = eng.ebp(x.to(dev), st, seed.to(dev), want_mwp=False, want_pooled=True)
                torch.cuda.synchronize()
                runs.append(pooled[0].detach().cpu())
            csv = tuning.record_launch_log(step, 0, dev)          # two sweeps
            rows = [l.strip().split(',') for l in open(csv)][1:]
            os.remove(csv)
            # nhalves, kh, chain steps, cfg, parts
            out['launches'] += [[int(r[3]), int(r[6]), int(r[7]), int(r[8]), int(r[11])] for r in rows]
            eng.set_tail_balance(0)
            step()                                                # no workspace: no parts
            eng.set_tail_balance(1)
            out['runs'].append({'n': n, 'e32': rel(want32, want), 'e_eng': [rel(r, want) for r in runs], 'finite': [bool(torch.isfinite(r).all()) for r in runs],
                                'repeat_equal': bool(torch.equal(runs[0], runs[1]))})
    finally:
        eng.close()
    print('ENGINE_LEG ' + json.dumps(out))


def test_engine_dual_and_chain_launches_with_parts(gpu_device):
    """The `bf16x6` net through the engine in a child process (the host rule's knobs are read once per process; here: parts on maps of any
    size, up to three, from two channel blocks / six K-steps each): its 3x3 128 -> 128 layers (eight channel blocks: parts of 3 + 3 + 2) and its
    256 -> 128 layer (slab mode, six passes) run as three parts -- plain, dual W / relu(W) and chain-epilogue launches, forward and backward-data,
    next to the fp32 kernels' tail-balanced launches on the same stream, workspace and counters.  The launch log says how many parts every
    launch really ran.  Pooled P[-2] of three and four images against float64; two sweeps bit for bit; without a workspace the same rule."""
    env = dict(os.environ)
    env.update(ENGINE_LEG_ENV)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    text = r.stdout.decode('utf-8', 'replace')
    assert r.returncode == 0, text + r.stderr.decode('utf-8', 'replace')
    out = json.loads([l for l in text.splitlines() if l.startswith('ENGINE_LEG ')][-1][len('ENGINE_LEG '):])
    for run in out['runs']:
        print(run)
        assert all(run['finite']) and run['repeat_equal'], run
        for e in run['e_eng']:
            assert e <= max(K_RATIO * run['e32'], FLOOR), run
    cut = [l for l in out['launches'] if l[3] == 9 and l[4] > 1]
    assert any(l[1] == 3 and l[4] == 3 for l in cut), 'no patch-mode launch ran as three parts'
    assert any(l[1] == 1 and l[4] == 3 for l in cut), 'no slab-mode launch ran as three parts'
    assert any(l[0] == 2 for l in cut), 'no dual W / relu(W) launch ran in parts'
    assert any(l[2] > 0 for l in cut), 'no launch with a chain epilogue ran in parts'
    assert all(l[4] == 1 for l in out['launches'] if l[3] != 9), 'the parts column is the bf16x6 kernel\'s'


if __name__ == '__main__':
    engine_leg()
