"""The two-accumulator (DUAL) instantiation of the bf16x6 GEMM kernel (conv_gemm_split.hip): the lean probe-forward launches -- the W tile and
the relu(W) tile of a convolution in one workgroup, relu(W) made from the W fragments in registers -- on the bf16 matrix pipe.

Two small nets of 1x1 convolutions on 7 x 7 maps, every one behind a BatchNorm + ReLU (a non-negative input: the planner makes them lean), at
the smallest shapes where each piece of the K loop can go wrong:
  Cin 32 -- one short pass (two of its three K-steps);  Cin 80 -- five K-steps, the second pass short and negated;  Cin 96 -- two whole passes;
  Cout 128 and 256 (one and two row tiles);  batch 4: M = 196 -- two m-tiles, the second a tail, tiles spanning image borders -- and batch 8.
The convolutions between them (Cout 80 / 96: not a multiple of 128) stay on the fp32 lean kernels, next to the bf16x6 launches on one stream.

Yardstick: pooled P[-2] of Engine.ebp against the float64 oracle and the rule of tests/test_gpu_layer_parity.py, e_eng <= max(4 e32, 2e-6), e32
the fp32 CPU oracle's own error.  (For these nets and seeds e32 is 2e-7 .. 5e-7 on the CPU: the fp32 oracle makes the float64 oracle's ReLU decisions, and
there is no pool.)  The engine runs in child processes -- the routing switch XFR_SPLIT_DUAL and the layer rule XFR_SPLIT_MIN_K1 (these layers
are shallower than the K = 256 the step's rule starts at) are read once per process -- one with the DUAL instantiation on, one with it off; the
launch log says which kernel every lean launch really took.
"""
import json
import os
import subprocess
import sys

if __name__ == '__main__':       # the child process (below): the paths pytest's conftest gives the suite
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]

import numpy as np
import pytest
import torch

import layer_nets as L
from parity_harness import FLOOR, K_RATIO
from xfr_amd.engine import Engine

pytestmark = pytest.mark.gpu

MODE = 'affineonly_with_prior'
BATCHES = (4, 8)


def _net(couts):
    """stem 3x3 16 -> 32; 1x1 32 -> couts[0]; -> 80; 1x1 80 -> couts[1]; -> 96; 1x1 96 -> couts[2]; a Linear head.  BatchNorm + ReLU after each."""
    def fwd(p):
        t = p.conv(0, 'stem', 32, 3, stride=1, pad=1, bias=False)
        t = p.relu_(p.batchnorm(t, 'stem_bn'))
        for i, (cout, bias) in enumerate(((couts[0], False), (80, True), (couts[1], True), (96, False), (couts[2], False))):
            t = p.conv(t, 'c%d' % i, cout, 1, bias=bias)
            t = p.relu_(p.batchnorm(t, 'c%d_bn' % i))
        return p.mark('classify', p.linear(t, 'fc', 5, (7, 7)))
    return fwd


# name -> (forward, the (Cout, K) of the launches the DUAL instantiation must take)
NETS = {
    'dual_a': (_net((128, 256, 128)), [(128, 32), (256, 80), (128, 96)]),
    'dual_b': (_net((256, 128, 256)), [(256, 32), (128, 80), (256, 96)]),
}
SEEDS = {'dual_a': 31, 'dual_b': 32}


def net_case(name, reseed=0):
    return L.NetCase(name, (16, 7, 7), NETS[name][0], 'lean two-accumulator launches on the bf16x6 kernel', SEEDS[name] + reseed)


def rel(a, ref):
    return float((a.double() - ref).abs().max()) / float(ref.abs().max())


def child():
    """All nets and batches through one engine each; prints one JSON object."""
    from xfr_amd import tuning
    dev = torch.device('cuda', 0)
    out = {}
    for name in sorted(NETS):
        case = net_case(name)
        eng = Engine(case.program(), 8, dev)
        res = {'runs': [], 'launches': []}
        try:
            eng.load_weights(case.params())
            eng.set_mode(MODE)
            eng.set_lean(1)
            eng.set_split_gemm(7)
            st = case.program().marks['classify']
            d = int(np.prod(eng.tensor_shape(st)))

            def sweep_twice(c, n, log):
                x = c.inputs(n, seed=1)
                g = torch.Generator().manual_seed(97 + n)
                seed = torch.rand((1, n, d), generator=g)
                P64, _, _ = c.oracle_P(x, seed[0], MODE, torch.float64)
                P32, _, _ = c.oracle_P(x, seed[0], MODE)
                want32, want = P32[-2].sum(dim=1), P64[-2].sum(dim=1)
                runs = []

                def step():
                    _, pooled = eng.ebp(x.to(dev), st, seed.to(dev), want_mwp=False, want_pooled=True)
                    torch.cuda.synchronize()
                    runs.append(pooled[0].detach().cpu())
                lean0 = eng.lean_launches()
                if log:
                    csv = tuning.record_launch_log(step, 0, dev)          # two sweeps
                    rows = [l.strip().split(',') for l in open(csv)][1:]
                    os.remove(csv)
                    # Cout, nhalves, K, M, cfg
                    res['launches'] += [[int(r[2]), int(r[3]), int(r[4]), int(r[5]), int(r[8])] for r in rows]
                else:
                    step()
                    step()
                return {'n': n, 'e32': rel(want32, want), 'e_eng': [rel(r, want) for r in runs], 'finite': [bool(torch.isfinite(r).all()) for r in runs],
                        'repeat_equal': bool(torch.equal(runs[0], runs[1])), 'lean_grew': eng.lean_launches() - lean0}, runs[0]
            first = {}
            for n in BATCHES:
                run, first[n] = sweep_twice(case, n, True)
                res['runs'].append(run)
            # other weights into the same engine: the bf16 planes of the packs must follow them
            other = net_case(name, reseed=100)
            eng.load_weights(other.params())
            run, got = sweep_twice(other, BATCHES[0], False)
            run['reloaded'] = True
            run['moved'] = rel(got, first[BATCHES[0]].double())
            res['runs'].append(run)
        finally:
            eng.close()
        out[name] = res
    print('SPLIT_DUAL ' + json.dumps(out))


_CHILD = {}


def run_child(dual):
    if dual not in _CHILD:
        env = dict(os.environ)
        env.update({'XFR_SPLIT_DUAL': str(dual), 'XFR_SPLIT_MIN_K1': '16'})
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
        text = r.stdout.decode('utf-8', 'replace')
        assert r.returncode == 0, text + r.stderr.decode('utf-8', 'replace')
        _CHILD[dual] = json.loads([l for l in text.splitlines() if l.startswith('SPLIT_DUAL ')][-1][len('SPLIT_DUAL '):])
    return _CHILD[dual]


def check_runs(res):
    for run in res['runs']:
        print(run)
        assert all(run['finite']), run
        assert run['repeat_equal'], 'two sweeps of the same input differ: %r' % (run,)
        assert run['lean_grew'] > 0, 'no lean launch: %r' % (run,)
        for e in run['e_eng']:
            assert e <= max(K_RATIO * run['e32'], FLOOR), run


@pytest.mark.parametrize('name', sorted(NETS))
def test_lean_launches_on_the_dual_instantiation_match_float64(gpu_device, name):
    """XFR_SPLIT_DUAL=1: every covered lean launch of the net -- each (Cout, Cin) at both batches -- shows configuration 9 with its nhalves column
    at 2, the uncovered ones an fp32 configuration; pooled P[-2] holds the float64 rule at batch 4 and 8; two sweeps are bit-identical; after a
    second load_weights the result follows the new weights."""
    res = run_child(1)[name]
    check_runs(res)
    lean9 = set((l[0], l[2], l[3]) for l in res['launches'] if l[1] == 2 and l[4] == 9)
    for cout, k in NETS[name][1]:
        for n in BATCHES:
            assert (cout, k, n * 49) in lean9, 'no bf16x6 two-accumulator launch for Cout %d, K %d, batch %d: %r' % (cout, k, n, sorted(lean9))
    assert any(l[1] == 2 and l[4] != 9 for l in res['launches']), 'the Cout 80 / 96 lean launches belong on the fp32 kernels'
    reloaded = [r for r in res['runs'] if r.get('reloaded')]
    assert len(reloaded) == 1 and reloaded[0]['moved'] > 1e-2, 'the second set of weights gives another map: %r' % (reloaded,)


@pytest.mark.parametrize('name', sorted(NETS))
def test_switched_off_the_lean_launches_stay_on_fp32(gpu_device, name):
    """XFR_SPLIT_DUAL=0: the same nets, no lean launch on configuration 9, the same rule."""
    res = run_child(0)[name]
    check_runs(res)
    assert not [l for l in res['launches'] if l[1] == 2 and l[4] == 9], 'a two-accumulator launch took the bf16x6 kernel with XFR_SPLIT_DUAL=0'
    assert any(l[1] == 2 for l in res['launches'])


if __name__ == '__main__':
    child()
