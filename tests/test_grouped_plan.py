"""Grouped convolutions in layer programs, without a GPU: the planner accepts every net of tests/grouped_nets.py in all four modes and lists each
grouped launch with its groups, per-group Ci / Co / K, M and the grouped kernel's configuration id; the grouped layer carries no chain while its dense
neighbours keep theirs; what a grouped layer may not be is refused with a message that says so; `groups` travels in the documented slot of the
64-byte op record; the torchvision family has torchvision's shapes and parameter counts; and the per-group dense form the kernel implements equals
F.conv2d(groups = g) and autograd's input gradient in float64."""
import ctypes
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grouped_nets as G
from xfr_amd import _lib
from xfr_amd.engine import MODES as MODE_IDS
from xfr_amd.program import OpDesc, Program

MODES = ('affineonly', 'affineonly_with_prior', 'norelu', 'all')
BATCH = 3
CFG_GROUP = 13
FWD = re.compile(r'^(fwd|probe) GROUPED op (\d+) \[(\d+) x (\d+) x (\d+)\] groups (\d+) Ci (\d+) Co (\d+) K (\d+) M (\d+) cfg (\d+)$')
BWD = re.compile(r'^bwd CONV_BWD src (\d+) dst (\d+) acc (\d) \[\d+ x \d+ x \d+\] K (\d+) groups (\d+) Ci (\d+) Co (\d+) M (\d+) cfg (\d+)$')
PHASE = re.compile(r'^bwd PHASE op (\d+) \((\d+),(\d+)\) kernel (\d+)x(\d+) cfg (\d+) K (\d+) M (\d+) origin \((\d+),(\d+)\) grid (\d+) x (\d+) groups (\d+) Ci (\d+) Co (\d+)$')


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', [c.name for c in G.CASES])
def test_describe_lists_the_grouped_launches(name, mode):
    case = G.BY_NAME[name]
    prog = case.program()
    text = prog.describe(mode, prog.marks['classify'], batch=BATCH)
    lines = text.splitlines()
    _, H, W, cin, cout, groups, k, s, p = case.grouped
    op = case.grouped_op(prog)
    oh, ow = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    # forward: one line per forward kind, the grouped K and the forward's M
    fwd = [FWD.match(ln) for ln in lines if ' GROUPED ' in ln]
    assert len(fwd) == 2 and all(fwd), text
    assert sorted(m.group(1) for m in fwd) == ['fwd', 'probe']
    for m in fwd:
        assert [int(v) for v in m.groups()[1:]] == [op, cout, oh, ow, groups, cin // groups, cout // groups, cin // groups * k * k, BATCH * oh * ow, CFG_GROUP], m.group(0)
    # no epilogue on the grouped layer in any forward, lean included; the dense layers keep theirs
    assert not any(re.match(r'^(fwd|probe|lean-probe) CONV op %d ' % op, ln) for ln in lines), text
    assert any(re.match(r'^fwd CONV op \d+ .* SIG', ln) for ln in lines) and any(re.match(r'^probe CONV op \d+ .* SIG', ln) for ln in lines), text
    # backward: the grouped layer's GEMM with the roles swapped, no chain on it
    bwd = [BWD.match(ln) for ln in lines if ln.startswith('bwd CONV_BWD') and ' groups ' in ln]
    assert len(bwd) == 1 and bwd[0], text
    v = [int(x) for x in bwd[0].groups()]
    assert v[3:7] == [cout // groups * k * k, groups, cout // groups, cin // groups] and v[8] == CFG_GROUP
    assert ' SIG' not in bwd[0].group(0)
    for prefix in ('bwd', 'observed-bwd', 'lean-bwd'):
        for ln in lines:
            if ln.startswith(prefix + ' CONV_BWD') and ' SIG' in ln:
                assert ' groups ' not in ln
                src = int(re.match(r'^\S+ CONV_BWD src (\d+)', ln).group(1))
                assert src != op + 1, ln                    # tensor op + 1 is the grouped layer's output: its GEMM carries nothing
    dense_chains = [ln for ln in lines if ln.startswith('bwd CONV_BWD') and ' SIG' in ln]
    assert dense_chains, text                                # ... while a dense neighbour's does
    if s == 1:
        assert v[7] == 2 * BATCH * H * W and not [ln for ln in lines if ln.startswith('bwd PHASE')]
    elif k > 1:
        got = [PHASE.match(ln) for ln in lines if ln.startswith('bwd PHASE')]
        want = G.phases(case)
        assert len(got) == len(want) == 4 and all(got), text
        for m, ph in zip(got, want):
            u = [int(x) for x in m.groups()]
            assert u[0] == op and u[1:5] == [ph['r'], ph['c'], ph['ka'], ph['kb']] and u[5] == CFG_GROUP and u[6] == ph['K'] == cout // groups * ph['ka'] * ph['kb']
            assert u[7] == 2 * BATCH * ph['nq'] * ph['nu'] and u[8:12] == [ph['ih0'], ph['iw0'], ph['nq'], ph['nu']]
            assert u[12:] == [groups, cout // groups, cin // groups]
    else:
        assert v[7] == 2 * BATCH * oh * ow and v[2] == 1     # the strided 1x1: M on the sampled grid, accumulating onto the zero fill


def test_lean_plan_keeps_the_grouped_layer_literal():
    """At a batch that is a multiple of 4 the dense neighbours go lean; no lean epilogue and no lean chain belongs to the grouped layer."""
    case = G.BY_NAME['resnext_block']
    prog = case.program()
    op = case.grouped_op(prog)
    text = prog.describe('affineonly_with_prior', prog.marks['classify'], batch=4)
    lean = [ln for ln in text.splitlines() if ln.startswith('lean-probe CONV')]
    assert lean and not any(ln.startswith('lean-probe CONV op %d ' % op) for ln in lean), text
    assert re.search(r'^lean convolutions [1-9]', text, re.M)


def _describe_status(prog, out, in_shape):
    lib = _lib.load()
    need = ctypes.c_size_t()
    st = lib.xfr_plan_describe(prog.op_array(), len(prog.ops), len(prog.weight_names), in_shape[0], in_shape[1], in_shape[2], 1,
                               MODE_IDS['affineonly_with_prior'], out, None, 0, ctypes.byref(need))
    return st, lib.xfr_last_error().decode()


def _net(cin0, cout, groups, first_groups=1, linear_groups=0, mfm=False):
    prog = Program((cin0 if first_groups > 1 else 3, 8, 8))
    t = prog.conv(0, 'conv0', cin0, 3, stride=1, pad=1, groups=first_groups)
    t = prog.relu_(t)
    t = prog.conv(t, 'g', cout, 3, stride=1, pad=1, groups=groups)
    if mfm:
        t = prog.g_maxhalves(prog.split(t))
    else:
        t = prog.relu_(t)
    out = prog.linear(t, 'fc', 5, (8, 8))
    if linear_groups:
        prog.ops[-1].ceil_mode = linear_groups
    return prog, out


@pytest.mark.parametrize('what,kwargs,status,fragments', [
    ('cin', dict(cin0=30, cout=32, groups=4), 'XFR_INVALID_ARG', ('30 input channels', 'groups 4')),
    ('cout', dict(cin0=32, cout=30, groups=4), 'XFR_INVALID_ARG', ('30 output channels', 'groups 4')),
    ('linear', dict(cin0=32, cout=32, groups=1, linear_groups=2), 'XFR_UNSUPPORTED_LAYER', ('groups 2', 'Linear')),
    ('first', dict(cin0=8, cout=8, groups=1, first_groups=2), 'XFR_UNSUPPORTED_LAYER', ('groups 2', 'first layer')),
    ('mfm', dict(cin0=32, cout=32, groups=4, mfm=True), 'XFR_UNSUPPORTED_LAYER', ('groups 4', 'MaxFeatureMap')),
])
def test_refusals(what, kwargs, status, fragments):
    prog, out = _net(**kwargs)
    st, msg = _describe_status(prog, out, prog.in_shape)
    assert st == getattr(_lib, status), (st, msg)
    assert all(f in msg for f in fragments) and re.search(r'op \d+', msg), msg


def test_negative_groups_is_refused():
    prog, out = _net(32, 32, 1)
    prog.ops[2].ceil_mode = -2
    st, msg = _describe_status(prog, out, prog.in_shape)
    assert st == _lib.XFR_INVALID_ARG and 'groups must be >= 1' in msg and '-2' in msg, (st, msg)


def test_strided_padding_rule_applies_to_grouped_layers():
    prog = Program((16, 12, 12))
    t = prog.relu_(prog.conv(0, 'conv0', 16, 3, stride=1, pad=1))
    t = prog.relu_(prog.conv(t, 'down', 16, 3, stride=2, pad=2, groups=4))
    out = prog.linear(t, 'fc', 5, (7, 7))
    st, msg = _describe_status(prog, out, prog.in_shape)
    assert st == _lib.XFR_UNSUPPORTED_LAYER and 'pad <= kernel - stride' in msg, (st, msg)


def test_groups_travels_in_the_documented_slot():
    assert ctypes.sizeof(OpDesc) == 64
    prog = Program((8, 6, 6))
    t = prog.conv(0, 'conv0', 8, 3, pad=1)
    a = prog.conv(t, 'a', 16, 3, stride=1, pad=1, bias=False, groups=4)
    b = prog.conv(a, 'b', 16, 3, pad=1)
    c = prog.conv(b, 'c', 16, 1, groups=1)
    assert prog.ops[a - 1].ceil_mode == 4 and prog.ops[b - 1].ceil_mode == 0 and prog.ops[c - 1].ceil_mode == 0 and prog.ops[0].ceil_mode == 0
    assert prog.tensor_channels()[a] == 16
    assert prog.module_repr(a - 1) == str(torch.nn.Conv2d(8, 16, 3, stride=1, padding=1, groups=4, bias=False))
    assert 'groups=4' in prog.module_repr(a - 1) and 'groups' not in prog.module_repr(b - 1)
    assert prog.module_repr(b - 1) == str(torch.nn.Conv2d(16, 16, 3, stride=1, padding=1))


def test_resnext_family():
    """torchvision's key set, shapes and parameter counts; a plan with 16 grouped layers, three of them by four phases."""
    from xfr_amd.models import tv_resnet
    net = tv_resnet.resnext50_32x4d()
    sd = net.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    assert shapes['layer1.0.conv1.weight'] == (128, 64, 1, 1)
    assert shapes['layer1.0.conv2.weight'] == (128, 4, 3, 3)
    assert shapes['layer1.0.conv3.weight'] == (256, 128, 1, 1)
    assert shapes['layer2.0.conv2.weight'] == (256, 8, 3, 3)
    assert shapes['layer3.5.conv2.weight'] == (512, 16, 3, 3)
    assert shapes['layer4.2.conv2.weight'] == (1024, 32, 3, 3)
    assert shapes['layer4.0.downsample.0.weight'] == (2048, 1024, 1, 1) and shapes['fc.weight'] == (1000, 2048)
    ref = tv_resnet.resnet50()
    assert set(sd) == set(ref.state_dict())                  # the same names as ResNet-50, which test_strided_plan.py holds to torchvision's

    def count(m):
        return sum(int(np.prod(s)) for n, s, kind in m.param_specs() if kind in ('conv_w', 'bn_w', 'bn_b', 'fc_w', 'fc_b'))
    assert count(net) == 25028904
    assert count(tv_resnet.wide_resnet50_2()) == 68883240
    assert count(ref) == 25557032
    assert {k: tuple(v.shape) for k, v in tv_resnet.wide_resnet50_2().state_dict().items()}['layer1.0.conv2.weight'] == (128, 128, 3, 3)
    assert tv_resnet.resnext101_32x8d(num_classes=10).param_specs()[-2][1] == (10, 2048)
    d101 = dict((n, s) for n, s, _ in tv_resnet.resnext101_32x8d().param_specs())
    assert d101['layer3.22.conv2.weight'] == (1024, 32, 3, 3) and d101['layer1.0.conv2.weight'] == (256, 8, 3, 3)
    d64 = dict((n, s) for n, s, _ in tv_resnet.resnext101_64x4d().param_specs())
    assert d64['layer1.0.conv2.weight'] == (256, 4, 3, 3)
    with pytest.raises(ValueError, match='BasicBlock'):
        tv_resnet.TVResnet('basic', (2, 2, 2, 2), groups=32, width_per_group=4)
    prog = net.build_program()
    text = prog.describe('affineonly_with_prior', prog.marks['classify'], batch=2)
    fwd = [FWD.match(ln) for ln in text.splitlines() if ln.startswith('fwd GROUPED')]
    assert len(fwd) == 16 and all(fwd)
    assert all(int(m.group(6)) == 32 and int(m.group(11)) == CFG_GROUP for m in fwd)
    ph = [PHASE.match(ln) for ln in text.splitlines() if ln.startswith('bwd PHASE')]
    assert len(ph) == 12 and all(ph) and len(set(m.group(1) for m in ph)) == 3
    names = prog.layernames('norelu', prog.marks['classify'])
    assert 'Conv2d(128, 128, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), groups=32, bias=False)' in names


def test_synth_weights_of_a_grouped_layer():
    """synth_state_dict draws conv weights with torchvision's kaiming fan_out, cout * kh * kw, which a grouped shape leaves as it is; the grouped
    shape itself comes from param_specs."""
    from xfr_amd import synth
    from xfr_amd.models import tv_resnet
    net = tv_resnet.TVResnet('bottleneck', (1, 1, 1, 1), num_classes=7, width=16, in_shape=(3, 40, 36), groups=4, width_per_group=16)
    sd = synth.synth_state_dict(net, seed=5)
    w = sd['layer2.0.conv2.weight']
    assert tuple(w.shape) == (32, 8, 3, 3)
    assert abs(float(w.std()) / np.sqrt(2.0 / (9 * 32)) - 1) < 0.1


@pytest.mark.parametrize('name', [c.name for c in G.CASES])
def test_group_slab_form_equals_torch_float64(name):
    """Per-group dense convolution on channel slabs, and its flipped per-group backward (phases for the strided KxK layer), against
    F.conv2d(groups = g) and autograd's input gradient."""
    _, H, W, cin, cout, groups, k, s, p = G.BY_NAME[name].grouped
    g = torch.Generator().manual_seed(H * 100 + W + groups)
    x = torch.randn((2, cin, H, W), generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn((cout, cin // groups, k, k), generator=g, dtype=torch.float64)
    b = torch.randn((cout,), generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, b, stride=s, padding=p, groups=groups)
    got = G.grouped_conv_by_slabs(x.detach(), w, b, groups, s, p)
    assert float((got - y.detach()).abs().max()) <= 1e-12 * float(y.detach().abs().max())
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(y, x, dy)
    co = cout // groups
    if s == 1:
        dx = G.grouped_backward_by_slabs(dy, w, groups, p, (H, W))
    else:
        dx = torch.zeros_like(want)
        for ph in G.phases(G.BY_NAME[name]):
            q0, u0 = (ph['ih0'] + p - ph['r']) // s, (ph['iw0'] + p - ph['c']) // s
            pt, pl = ph['ka'] - 1 - q0, ph['kb'] - 1 - u0
            pb, pr = ph['nq'] + ph['ka'] - 1 - pt - dy.shape[2], ph['nu'] + ph['kb'] - 1 - pl - dy.shape[3]
            for gi in range(groups):
                sub = w[gi * co:(gi + 1) * co, :, ph['r']::s, ph['c']::s]
                assert sub.shape[0] * sub.shape[2] * sub.shape[3] == ph['K']
                d = F.pad(dy[:, gi * co:(gi + 1) * co], (pl, max(pr, 0), pt, max(pb, 0)))
                out = F.conv2d(d, sub.flip(2, 3).transpose(0, 1))[:, :, :ph['nq'], :ph['nu']]
                ci = cin // groups
                dx[:, gi * ci:(gi + 1) * ci, ph['ih0']::s, ph['iw0']::s] += out
    assert float((dx - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)


def test_catalogue_params_have_group_fan_in():
    case = G.BY_NAME['g8_c4']
    w = case.params()['gconv.weight']
    assert tuple(w.shape) == (32, 4, 3, 3)
    assert abs(float(w.std()) / (1.5 / np.sqrt(4 * 9)) - 1) < 0.15
    assert tuple(G.BY_NAME['dw_mult2'].params()['gconv.weight'].shape) == (24, 1, 3, 3)
