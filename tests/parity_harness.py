"""The float64 parity rule of the layer catalogues and the plumbing around it, stated once for test_gpu_layer_parity.py, test_gpu_layerwise_parity.py,
test_gpu_strided_parity.py, test_gpu_grouped_parity.py and test_gpu_depthwise_parity.py; test_gpu_grouped_direct.py holds single launches to the same rule.

The rule, for every tensor:  e_eng = max|engine - fp64| / max|fp64|,  e32 = max|fp32 oracle - fp64| / max|fp64| (the reference's own precision on the
same tensor), and  e_eng <= max(K_RATIO * e32 + cond, FLOOR);  cond is zero except on layerwise rows (layerwise_inputs.one_element_cond).  K_RATIO and
FLOOR were chosen before measuring (test_gpu_layer_parity.py's docstring) and kept.

A test module holds one Harness: its engines (one per net and max_batch, closed by finish), its oracle sweeps, and the report finish writes.
"""
import csv
import json
import os

import numpy as np
import torch

from xfr_amd.engine import Engine

K_RATIO = 4.0
FLOOR = 2e-6
MODES = ('affineonly', 'affineonly_with_prior', 'all', 'norelu')
FUSION_SEPARATE = 3 | (1 << 3) | (1 << 4) | (1 << 6) | (1 << 7) | (1 << 8)
# (tag, batch, switches) of the un-observed sweeps of the strided, grouped and depthwise catalogues
SCHEDULES = [('default', 3, {}), ('default_b4', 4, {}), ('fusion0', 3, {'fusion': 0}), ('fusion_separate', 3, {'fusion': FUSION_SEPARATE}), ('literal_b4', 4, {'lean': 0})]
CFG_GROUP = 13              # the profile records' configuration of the grouped MFMA kernel
CFG_DEPTHWISE = 14          # ... of the depthwise kernel
KEEP_ON_13 = 1 << 10        # the fusion-mask bit that keeps depthwise launches on configuration 13
_written = set()            # the report files this process has written (Harness.finish)
_SETTERS = {'lean': ('set_lean', 1), 'split': ('set_split_gemm', 3), 'fusion': ('set_epilogue_fusion', 3), 'tail': ('set_tail_balance', 1)}


def _f64(v):
    return torch.as_tensor(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v)).double()


class Harness(object):
    def __init__(self, switches=('lean', 'fusion'), report_all=True, print_check=False, print_rule=False):
        """switches: the engine switches `apply` sets.  report_all False: `rule` leaves a callable ref32 uncalled where e_eng <= FLOOR.  print_check,
        print_rule: print every comparison of that form."""
        self.switches, self.report_all, self.print_check, self.print_rule = switches, report_all, print_check, print_rule
        self.report, self.engines, self.oracles = {}, {}, {}

    def engine(self, case, device, max_batch=8):
        key = (case.name, max_batch)
        if key not in self.engines:
            e = Engine(case.program(), max_batch, device)
            e.load_weights(case.params())
            self.engines[key] = e
        return self.engines[key]

    def seed(self, case, S, n, d, salt=0):
        g = torch.Generator().manual_seed(31 * case.seed + 7 * n + S + salt)
        return torch.rand((S, n, d), generator=g)

    def oracle(self, case, n, mode, salt):
        """(x, seed, P fp32 list, P fp64 list) of one sweep, computed once per session."""
        key = (case.name, n, mode, salt)
        if key not in self.oracles:
            x = case.inputs(n, seed=salt)
            tape, out = case.tape(x, torch.float64)
            seed = self.seed(case, 1, n, int(tape.T[out].shape[1]), salt)
            P64 = tape.backward(out, seed[0], mode, 1e-16)[0]
            P32 = case.oracle_P(x, seed[0], mode)[0]
            self.oracles[key] = (x, seed, P32, P64)
        return self.oracles[key]

    def apply(self, eng, sw):
        for name in self.switches:
            setter, default = _SETTERS[name]
            getattr(eng, setter)(sw.get(name, default))

    def finish(self, env_var, merge):
        """Close the engines; write the report to the file `env_var` names, on top of what is there if `merge`.  Whatever `merge` says, what an earlier
        module of THIS session wrote there stays: the module that starts the file afresh (merge False) does not come first in every collection order."""
        for e in self.engines.values():
            e.close()
        self.engines.clear()
        path = os.environ.get(env_var)
        if path:
            out = {}
            if (merge or os.path.abspath(path) in _written) and os.path.exists(path):
                with open(path) as f:
                    out = json.load(f)
            _written.add(os.path.abspath(path))
            out.update(self.report)
            with open(path, 'w') as f:
                json.dump(out, f, indent=0, sort_keys=True)

    def _compare(self, bad, key, got, ref32, ref64, cond, scale, with_cond, show):
        """The rule on a finite `got` of ref64's shape, both float64, errors relative to `scale`."""
        e_eng = float((got - ref64).abs().max()) / scale
        if callable(ref32):
            if e_eng <= FLOOR and not self.report_all:
                self.report[key] = (e_eng, None, float(cond))
                return
            ref32 = ref32()
        e32 = float((_f64(ref32) - ref64).abs().max()) / scale
        self.report[key] = (e_eng, e32, float(cond)) if with_cond else (e_eng, e32)
        if show:
            print('%s e_eng %.3e e32 %.3e' % (key, e_eng, e32) + (' cond %.3e' % cond if with_cond else ''))
        if e_eng > max(K_RATIO * e32 + cond, FLOOR):
            i = int((got - ref64).abs().argmax())
            idx = tuple(int(v) for v in np.unravel_index(i, tuple(ref64.shape)))
            bad.append('%s: e_eng %.3e > max(%g x e32 %.3e + cond %.3e, %g); worst element %s: engine %.9g, fp64 %.9g' % (
                key, e_eng, K_RATIO, e32, cond, FLOOR, idx, float(got.reshape(-1)[i]), float(ref64.reshape(-1)[i])))

    def _usable(self, bad, key, got, ref64):
        if tuple(got.shape) != tuple(ref64.shape):
            bad.append('%s: shape %s vs %s' % (key, tuple(got.shape), tuple(ref64.shape)))
        elif not bool(torch.isfinite(got).all()):
            bad.append('%s: non-finite values' % key)
        else:
            return True
        return False

    def check(self, bad, key, got, p32, p64):
        """Record (e_eng, e32) under key; append a message to `bad` when the engine misses the rule."""
        got, p64 = _f64(got), _f64(p64)
        if self._usable(bad, key, got, p64):
            self._compare(bad, key, got, p32, p64, 0.0, max(float(p64.abs().max()), 1e-300), False, self.print_check)

    def rule(self, bad, key, got, ref32, ref64, cond=0.0):
        """Record (e_eng, e32, cond) under key; append a message to `bad` when `got` misses the rule against the float64 truth.  ref32 may be a
        function: the float32 tape's tensor is only needed where e_eng exceeds FLOOR (or for the report), and costs a sweep of the tape.  A truth that
        is identically zero asks for an identically zero `got` and records nothing."""
        got, ref64 = _f64(got), _f64(ref64)
        if not self._usable(bad, key, got, ref64):
            return
        scale = float(ref64.abs().max())
        if scale != 0:
            self._compare(bad, key, got, ref32, ref64, cond, scale, True, self.print_rule)
        elif float(got.abs().max()) != 0:
            bad.append('%s: the truth is identically zero, the engine has max|.| %.3e' % (key, float(got.abs().max())))


def run_every_firing(h, case, device):
    """Engine.ebp_firing(k) for every firing k including k == firing_count (the P[-1] gather), four subtree modes, one and three images."""
    eng = h.engine(case, device)
    st = case.program().marks['classify']
    bad = []
    for n in (1, 3):
        for mode in MODES:
            eng.set_mode(mode)
            x, seed, P32, P64 = h.oracle(case, n, mode, 0)
            nf = eng.firing_count(st)
            assert nf + 1 == len(P64), (case.name, nf, len(P64))
            xd, sd = x.to(device), seed.to(device)
            for k in range(nf + 1):
                h.check(bad, '%s/%s/n%d/P[%d]' % (case.name, mode, n, k), eng.ebp_firing(xd, st, sd, k), P32[k], P64[k])
    assert not bad, '\n'.join(bad)


def run_schedule_pooled(h, case, device, mode, schedules):
    """Engine.ebp(want_pooled=True), the un-observed sweep, against the float64 pooled P[-2] under every (tag, batch, switches) of `schedules`."""
    eng = h.engine(case, device)
    eng.set_mode(mode)
    st = case.program().marks['classify']
    bad = []
    try:
        for tag, n, sw in schedules:
            x, seed, P32, P64 = h.oracle(case, n, mode, 1)
            h.apply(eng, sw)
            _, pooled = eng.ebp(x.to(device), st, seed.to(device), want_mwp=False, want_pooled=True)
            torch.cuda.synchronize()
            h.check(bad, '%s/%s/%s' % (case.name, mode, tag), pooled[0], P32[-2].sum(dim=1), P64[-2].sum(dim=1))
    finally:
        h.apply(eng, {})
    assert not bad, '\n'.join(bad)


def profiled_sweep(eng, case, device, path, n, streams):
    """One un-observed sweep of `streams` seeds with the per-launch profile records appended to `path` -> the records as lists of strings:
    (Cout, nhalves, K, M, kh, stride, out_stride, relu_in, accumulate, ms, TFLOP/s, cfg)."""
    st = case.program().marks['classify']
    x = case.inputs(n, seed=1).to(device)
    d = int(np.prod(eng.tensor_shape(st)))
    seed = torch.rand((streams, n, d), generator=torch.Generator().manual_seed(5)).to(device)
    eng.set_profile(True)
    eng.profile_csv(path)
    try:
        eng.ebp(x, st, seed, want_mwp=False, want_pooled=True)
        torch.cuda.synchronize()
    finally:
        eng.profile_csv(None)
        eng.set_profile(False)
    with open(path) as f:
        return [r for r in csv.reader(f) if r]


def by_cfg(rows, cfg):
    return [[int(v) for v in r[:9]] for r in rows if int(r[11]) == cfg]
