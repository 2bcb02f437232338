"""Depthwise layers in layer programs, without a GPU: the planner accepts every net of tests/depthwise_nets.py in all four modes and lists each
depthwise launch as the grouped launch it plans -- groups C, Ci 1, Co m, the K of one group, configuration id 13: which of the two grouped kernels
takes a launch is the launcher's decision (conv_depthwise.hip first), not the plan's, so these lines are what they were before that kernel existed.
models/mobilenet.py has the parameter shapes of a plain-torch statement of the same net.  No tolerance lives in this file."""
import re

import pytest
import torch
import torch.nn as nn

import depthwise_nets as D
from grouped_nets import phases

MODES = ('affineonly', 'affineonly_with_prior', 'norelu', 'all')
BATCH = 3
CFG_GROUP = 13
FWD = re.compile(r'^(fwd|probe) GROUPED op (\d+) \[(\d+) x (\d+) x (\d+)\] groups (\d+) Ci (\d+) Co (\d+) K (\d+) M (\d+) cfg (\d+)$')
BWD = re.compile(r'^bwd CONV_BWD src (\d+) dst (\d+) acc (\d) \[\d+ x \d+ x \d+\] K (\d+) groups (\d+) Ci (\d+) Co (\d+) M (\d+) cfg (\d+)$')
PHASE = re.compile(r'^bwd PHASE op (\d+) \((\d+),(\d+)\) kernel (\d+)x(\d+) cfg (\d+) K (\d+) M (\d+) origin \((\d+),(\d+)\) grid (\d+) x (\d+) groups (\d+) Ci (\d+) Co (\d+)$')


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', [c.name for c in D.CASES])
def test_describe_lists_the_depthwise_launches(name, mode):
    case = D.BY_NAME[name]
    prog = case.program()
    text = prog.describe(mode, prog.marks['classify'], batch=BATCH)
    lines = text.splitlines()
    _, H, W, cin, cout, groups, k, s, p = case.grouped
    op = case.grouped_op(prog)
    oh, ow = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    fwd = [m for m in (FWD.match(ln) for ln in lines if ' GROUPED ' in ln) if m and int(m.group(2)) == op]
    assert sorted(m.group(1) for m in fwd) == ['fwd', 'probe'], text
    for m in fwd:
        assert [int(v) for v in m.groups()[1:]] == [op, cout, oh, ow, groups, cin // groups, cout // groups, cin // groups * k * k, BATCH * oh * ow, CFG_GROUP], m.group(0)
    assert all(int(m.group(11)) == CFG_GROUP for m in (FWD.match(ln) for ln in lines if ' GROUPED ' in ln)), text
    bwd = [BWD.match(ln) for ln in lines if ln.startswith('bwd CONV_BWD') and ' groups ' in ln]
    assert all(bwd) and all(int(m.group(9)) == CFG_GROUP for m in bwd), text
    if s == 1:
        mine = [m for m in bwd if int(m.group(1)) == op + 1]
        assert len(mine) == 1, text
        v = [int(x) for x in mine[0].groups()]
        assert v[3:8] == [cout // groups * k * k, groups, cout // groups, cin // groups, 2 * BATCH * H * W]
    elif k > 1:
        got = [m for m in (PHASE.match(ln) for ln in lines if ln.startswith('bwd PHASE')) if m and int(m.group(1)) == op]
        want = phases(case)
        assert len(got) == len(want) == 4, text
        for m, ph in zip(got, want):
            u = [int(x) for x in m.groups()]
            assert u[1:5] == [ph['r'], ph['c'], ph['ka'], ph['kb']] and u[5] == CFG_GROUP and u[6] == ph['K']
            assert u[7] == 2 * BATCH * ph['nq'] * ph['nu'] and u[12:] == [groups, cout // groups, cin // groups]
    else:
        mine = [m for m in bwd if int(m.group(1)) == op + 1]
        assert len(mine) == 1 and int(mine[0].group(8)) == 2 * BATCH * oh * ow and int(mine[0].group(3)) == 1, text


def test_module_repr_prints_groups():
    case = D.BY_NAME['dw_bias']
    prog = case.program()
    op = case.grouped_op(prog)
    assert prog.module_repr(op) == str(nn.Conv2d(20, 20, 3, stride=1, padding=1, groups=20))
    assert 'groups=20' in prog.module_repr(op)
    case = D.BY_NAME['mult3']
    prog = case.program()
    assert prog.module_repr(case.grouped_op(prog)) == str(nn.Conv2d(8, 24, 3, stride=1, padding=1, groups=8, bias=False))


class _TorchMobileNetV1(nn.Module):
    """The same net in plain torch, for its state_dict: the attribute paths are the names models/mobilenet.py documents."""
    WIDTHS = (64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 512, 1024, 1024)
    STRIDES = (1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1)

    def __init__(self, num_classes, alpha, last_map, gdc):
        super(_TorchMobileNetV1, self).__init__()
        c = int(32 * alpha)
        self.conv1 = nn.Conv2d(3, c, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(c)
        blocks = []
        for wd, s in zip(self.WIDTHS, self.STRIDES):
            co = int(wd * alpha)
            b = nn.Module()
            b.dw = nn.Conv2d(c, c, 3, stride=s, padding=1, groups=c, bias=False)
            b.dw_bn = nn.BatchNorm2d(c)
            b.pw = nn.Conv2d(c, co, 1, bias=False)
            b.pw_bn = nn.BatchNorm2d(co)
            blocks.append(b)
            c = co
        self.blocks = nn.ModuleList(blocks)
        if gdc:
            self.gdc = nn.Conv2d(c, c, last_map, groups=c, bias=False)
            self.gdc_bn = nn.BatchNorm2d(c)
        self.fc = nn.Linear(c, num_classes)


@pytest.mark.parametrize('alpha,head,in_shape,last_map', [(1.0, 'avgpool', (3, 224, 224), (7, 7)), (0.25, 'avgpool', (3, 224, 224), (7, 7)),
                                                         (1.0, 'gdc', (3, 224, 224), (7, 7)), (0.5, 'gdc', (3, 112, 112), (4, 4))])
def test_mobilenet_v1_family(alpha, head, in_shape, last_map):
    from xfr_amd import synth
    from xfr_amd.models import mobilenet
    net = mobilenet.MobileNetV1(num_classes=1000, alpha=alpha, in_shape=in_shape, head=head)
    assert net.last_map() == last_map and net.feature_dim == int(1024 * alpha)
    ref = _TorchMobileNetV1(1000, alpha, last_map, head == 'gdc')
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert list(got) == list(want)
    assert got == want
    sd = synth.synth_state_dict(net, seed=3)
    net.load_state_dict(sd)
    assert torch.equal(net.state_dict()['blocks.12.dw.weight'], sd['blocks.12.dw.weight'])
    prog = net.build_program()
    text = prog.describe('affineonly_with_prior', prog.marks['classify'], batch=2)
    fwd = [FWD.match(ln) for ln in text.splitlines() if ln.startswith('fwd GROUPED')]
    n_dw = 13 + (1 if head == 'gdc' else 0)
    assert len(fwd) == n_dw and all(fwd)
    assert all(int(m.group(6)) == int(m.group(3)) and int(m.group(7)) == 1 and int(m.group(8)) == 1 and int(m.group(11)) == CFG_GROUP for m in fwd)
    assert [int(m.group(9)) for m in fwd][:13] == [9] * 13
    if head == 'gdc':
        assert int(fwd[-1].group(9)) == last_map[0] * last_map[1] and fwd[-1].group(4) == fwd[-1].group(5) == '1'
    ph = [PHASE.match(ln) for ln in text.splitlines() if ln.startswith('bwd PHASE')]
    assert len(ph) == 16 and all(ph) and len(set(m.group(1) for m in ph)) == 4          # the four strided depthwise layers by four phases each
    names = prog.layernames('norelu', prog.marks['classify'])
    c = int(512 * alpha)
    assert 'Conv2d(%d, %d, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), groups=%d, bias=False)' % (c, c, c) in names
    assert names[0] == 'Linear(in_features=%d, out_features=1000, bias=True)' % int(1024 * alpha)


def test_makers_and_whitebox_wrapper_fields():
    from xfr_amd.models import mobilenet
    net = mobilenet.mobilenet_v1(alpha=0.25, num_classes=10)
    assert (net.num_classes, net.in_shape, net.head) == (10, (3, 224, 224), 'avgpool') and sorted(net.meta) == ['imageSize', 'mean', 'std']
    face = mobilenet.mobilefacenet_like(alpha=0.25)
    assert (face.num_classes, face.in_shape, face.head) == (128, (3, 112, 112), 'gdc')
    assert tuple(face.state_dict()['gdc.weight'].shape) == (256, 1, 4, 4) and tuple(face.state_dict()['fc.weight'].shape) == (128, 256)
    with pytest.raises(ValueError, match='head'):
        mobilenet.MobileNetV1(head='flatten')
