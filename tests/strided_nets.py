"""A catalogue of small layer programs around a strided KxK convolution behind the first layer, one net per boundary of its backward-data
pass by phases (xfr_amd/csrc/plan.hip PhaseRec): odd and even maps, rows the forward never read, two strided GEMMs into one tensor, a phase
without a second tap, a stride that leaves phases of one, two and four taps, and the ci-major K order.

Every net opens with a stride-1 3x3 + BatchNorm + ReLU and ends in a Linear head; the builders and NetCase are tests/layer_nets.py's.
`strided` names the convolution the net exists for, `phases(case)` lists what the formulas of the phase form
(layer_nets.phases) give for it.
"""
import layer_nets as L
from layer_nets import NetCase


def _single(cin0, cout, k, stride, pad, head_hw, bias=False):
    def fwd(p):
        """conv3x3 %d, BN, ReLU, a %dx%d / stride %d / pad %d convolution to %d channels, BN, ReLU, a Linear head on %d x %d."""
        t = p.conv(0, 'conv0', cin0, 3, stride=1, pad=1, bias=False)
        t = p.relu_(p.batchnorm(t, 'bn0'))
        t = p.conv(t, 'down', cout, k, stride=stride, pad=pad, bias=bias)
        t = p.relu_(p.batchnorm(t, 'down_bn'))
        return p.mark('classify', p.linear(t, 'fc', 5, head_hw))
    fwd.__doc__ = fwd.__doc__ % ((cin0, k, k, stride, pad, cout) + tuple(head_hw))
    return fwd


def _basic_block(p):
    """A stage-opening torchvision BasicBlock on a 14 x 10 map (-> 7 x 5): 3x3 s2 -> BN -> ReLU -> 3x3 -> BN, a 1x1 s2 projection + BN shortcut,
    functional add, ReLU: the phases of the 3x3 and the scatter of the 1x1 accumulate into one zero-filled tensor."""
    t = p.conv(0, 'conv0', 32, 3, stride=1, pad=1, bias=False)
    t = p.mark('block_in', p.relu_(p.batchnorm(t, 'bn0')))
    o = p.conv(t, 'b.conv1', 48, 3, stride=2, pad=1, bias=False)
    o = p.relu_(p.batchnorm(o, 'b.bn1'))
    o = p.conv(o, 'b.conv2', 48, 3, stride=1, pad=1, bias=False)
    o = p.batchnorm(o, 'b.bn2')
    sc = p.conv(t, 'b.downsample.0', 48, 1, stride=2, bias=False)
    sc = p.batchnorm(sc, 'b.downsample.1')
    t = p.relu_(p.g_add(o, sc))
    return p.mark('classify', p.linear(t, 'fc', 5, (7, 5)))


def _bottleneck_v15(p):
    """A stage-opening torchvision Bottleneck (v1.5: the stride on the 3x3) on a 13 x 9 map (-> 7 x 5): 1x1 -> 3x3 s2 -> 1x1, a 1x1 s2
    projection + BN shortcut, functional add, ReLU."""
    t = p.conv(0, 'conv0', 32, 3, stride=1, pad=1, bias=False)
    t = p.relu_(p.batchnorm(t, 'bn0'))
    o = p.conv(t, 'b.conv1', 16, 1, bias=False)
    o = p.relu_(p.batchnorm(o, 'b.bn1'))
    o = p.conv(o, 'b.conv2', 16, 3, stride=2, pad=1, bias=False)
    o = p.relu_(p.batchnorm(o, 'b.bn2'))
    o = p.conv(o, 'b.conv3', 64, 1, bias=False)
    o = p.batchnorm(o, 'b.bn3')
    sc = p.conv(t, 'b.downsample.0', 64, 1, stride=2, bias=False)
    sc = p.batchnorm(sc, 'b.downsample.1')
    t = p.relu_(p.g_add(o, sc))
    return p.mark('classify', p.linear(t, 'fc', 5, (7, 5)))


class StridedCase(NetCase):
    def __init__(self, name, in_shape, forward, target, seed, strided):
        NetCase.__init__(self, name, in_shape, forward, target, seed)
        self.strided = strided          # (weight prefix, H, W of its input, cout, kernel, stride, pad)


CASES = [
    StridedCase('s2_odd', (32, 15, 13), _single(32, 48, 3, 2, 1, (8, 7)), '3x3/s2/p1 on an odd map: four phases of 1, 2, 2 and 4 taps', 31,
                ('down', 15, 13, 48, 3, 2, 1)),
    StridedCase('s2_valid', (32, 10, 8), _single(32, 48, 3, 2, 0, (4, 3)), '3x3/s2/p0: input row 9 and column 7 are never read and get zero gradient', 32,
                ('down', 10, 8, 48, 3, 2, 0)),
    StridedCase('basic_block', (32, 14, 10), _basic_block, 'two strided GEMMs (3x3 phases, 1x1 scatter) into one zero-filled tensor', 33,
                ('b.conv1', 14, 10, 48, 3, 2, 1)),
    StridedCase('bottleneck_v15', (32, 13, 9), _bottleneck_v15, 'the stride on the 3x3 between two 1x1 layers, Cout 16 (one K-step per tap)', 34,
                ('b.conv2', 13, 9, 16, 3, 2, 1)),
    StridedCase('s3_5x5', (32, 11, 9), _single(32, 32, 5, 3, 2, (4, 3), bias=True), '5x5/s3/p2: nine phases of 2x2, 2x2, 2x1, ... 1x1 taps, unequal leading paddings', 35,
                ('down', 11, 9, 32, 5, 3, 2)),
    StridedCase('patch2', (32, 12, 10), _single(32, 64, 2, 2, 0, (6, 5)), '2x2/s2/p0 (patchify): four one-tap phases', 36,
                ('down', 12, 10, 64, 2, 2, 0)),
    StridedCase('mid7', (24, 17, 12), _single(24, 40, 7, 2, 3, (9, 6)), '7x7/s2/p3 behind 24 channels (Cin % 16 != 0 forward, Cout % 16 != 0: ci-major phase packs)', 37,
                ('down', 17, 12, 40, 7, 2, 3)),
]
BY_NAME = {c.name: c for c in CASES}


def phases(case):
    """The phase launches of the net's strided layer (layer_nets.phases)."""
    _, H, W, cout, k, s, p = case.strided
    return L.phases(H, W, cout, k, s, p)
