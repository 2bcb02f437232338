"""A catalogue of small layer programs around a grouped convolution (Conv2d(groups = G): xfr_amd/csrc/conv_group.hip), one net per boundary of the
grouped kernel and of its per-group packs: row blocks padded from 4, 2 or 1 channel to 16, a ragged last row block, Ci != Co (the backward-data
GEMM swaps them), K that is no multiple of 4, a strided grouped 1x1 (scatter store), a bias, the phases of a strided grouped 3x3 next to a dense
scatter, and a batch prefix.

Every net opens with a dense 3x3 + BatchNorm + ReLU and ends in a Linear head; NetCase and the tape builder are tests/layer_nets.py's, whose `conv`
takes `groups` (oracle/ebp_oracle.py Tape.conv passes it to F.conv2d).  `grouped` names the layer the net exists for.
"""
import torch
import torch.nn.functional as F

import layer_nets as L
from layer_nets import NetCase


def _single(cin0, cout, groups, k, stride, pad, head_hw, bias=False):
    def fwd(p):
        """conv3x3 %d, BN, ReLU, a %dx%d / stride %d / pad %d convolution in %d groups to %d channels, BN, ReLU, a Linear head on %d x %d."""
        t = p.conv(0, 'conv0', cin0, 3, stride=1, pad=1, bias=False)
        t = p.relu_(p.batchnorm(t, 'bn0'))
        t = p.conv(t, 'gconv', cout, k, stride=stride, pad=pad, bias=bias, groups=groups)
        t = p.relu_(p.batchnorm(t, 'gconv_bn'))
        return p.mark('classify', p.linear(t, 'fc', 5, head_hw))
    fwd.__doc__ = fwd.__doc__ % ((cin0, k, k, stride, pad, groups, cout) + tuple(head_hw))
    return fwd


def _resnext_block(p):
    """A stage-opening ResNeXt bottleneck on a 13 x 9 map (-> 7 x 5): 1x1 -> grouped 3x3 s2 (G 4, inner width 16) -> 1x1, a 1x1 s2 projection + BN
    shortcut, functional add, ReLU: the phases of the grouped layer and the dense scatter of the projection accumulate into one zero-filled tensor."""
    t = p.conv(0, 'conv0', 32, 3, stride=1, pad=1, bias=False)
    t = p.relu_(p.batchnorm(t, 'bn0'))
    o = p.conv(t, 'b.conv1', 16, 1, bias=False)
    o = p.relu_(p.batchnorm(o, 'b.bn1'))
    o = p.conv(o, 'b.conv2', 16, 3, stride=2, pad=1, bias=False, groups=4)
    o = p.relu_(p.batchnorm(o, 'b.bn2'))
    o = p.conv(o, 'b.conv3', 64, 1, bias=False)
    o = p.batchnorm(o, 'b.bn3')
    sc = p.conv(t, 'b.downsample.0', 64, 1, stride=2, bias=False)
    sc = p.batchnorm(sc, 'b.downsample.1')
    t = p.relu_(p.g_add(o, sc))
    return p.mark('classify', p.linear(t, 'fc', 5, (7, 5)))


class GroupedCase(NetCase):
    def __init__(self, name, in_shape, forward, target, seed, grouped, batch=None):
        NetCase.__init__(self, name, in_shape, forward, target, seed)
        self.grouped = grouped          # (weight prefix, H, W of its input, Cin, cout, groups, kernel, stride, pad)
        self.batch = batch              # the batch the net is in the catalogue for (None: any)

    def grouped_op(self, prog=None):
        """Index of the grouped layer in the program."""
        prog = prog or self.program()
        return [i for i, o in enumerate(prog.ops) if o.w_weight >= 0 and prog.weight_names[o.w_weight] == self.grouped[0] + '.weight'][0]


CASES = [
    GroupedCase('g8_c4', (32, 15, 13), _single(32, 32, 8, 3, 1, 1, (15, 13)), 'Ci = Co = 4: 4 of 16 rows of a row block live, ragged M, M % 4 != 0', 41,
                ('gconv', 15, 13, 32, 32, 8, 3, 1, 1)),
    GroupedCase('depthwise', (24, 11, 9), _single(24, 24, 24, 3, 1, 1, (11, 9)), 'Ci = Co = 1, K = 9 padded to 12', 42,
                ('gconv', 11, 9, 24, 24, 24, 3, 1, 1)),
    GroupedCase('dw_mult2', (12, 10, 7), _single(12, 24, 12, 3, 1, 1, (10, 7)), 'channel multiplier 2: Ci 1, Co 2, the backward roles swapped', 43,
                ('gconv', 10, 7, 12, 24, 12, 3, 1, 1)),
    GroupedCase('g2_ragged', (64, 9, 8), _single(64, 80, 2, 3, 1, 1, (9, 8)), 'Ci 32, Co 40: three row blocks per group, the last ragged, X shared by them', 44,
                ('gconv', 9, 8, 64, 80, 2, 3, 1, 1)),
    GroupedCase('g3_odd', (30, 11, 11), _single(30, 36, 3, 3, 1, 0, (9, 9)), 'Ci 10, Co 12: neither a multiple of 4, backward padding k - 1 - p = 2', 45,
                ('gconv', 11, 11, 30, 36, 3, 3, 1, 0)),
    GroupedCase('g4_1x1_s2', (32, 13, 9), _single(32, 48, 4, 1, 2, 0, (7, 5)), 'grouped 1x1 stride 2: the scattered backward store onto an odd map', 46,
                ('gconv', 13, 9, 32, 48, 4, 1, 2, 0)),
    GroupedCase('g4_5x5_bias', (16, 9, 12), _single(16, 32, 4, 5, 1, 2, (9, 12), bias=True), '5x5 p2 with bias (bias and bias_pos), 25 taps', 47,
                ('gconv', 9, 12, 16, 32, 4, 5, 1, 2)),
    GroupedCase('resnext_block', (32, 13, 9), _resnext_block, 'the four phases of a strided grouped 3x3 and a dense scatter into one zero-filled tensor', 48,
                ('b.conv2', 13, 9, 16, 16, 4, 3, 2, 1)),
    GroupedCase('g2_prefix', (32, 15, 13), _single(32, 32, 2, 3, 1, 1, (15, 13)), 'as g8_c4 with G 2; run at batch 3 on an engine of max_batch 8: in_nb > NB', 49,
                ('gconv', 15, 13, 32, 32, 2, 3, 1, 1), batch=3),
]
BY_NAME = {c.name: c for c in CASES}


def phases(case):
    """The phase launches of the net's strided grouped KxK layer (layer_nets.phases), with the K of ONE group."""
    _, H, W, cin, cout, G, k, s, p = case.grouped
    return L.phases(H, W, cout // G, k, s, p)


def grouped_conv_by_slabs(x, w, bias, groups, stride, pad):
    """The form the engine implements, restated: group g is a dense convolution of the input channel slab [g Ci, (g + 1) Ci) with the weight rows
    [g Co, (g + 1) Co) into the output channel slab of the same index."""
    co = w.shape[0] // groups
    ci = w.shape[1]
    outs = []
    for g in range(groups):
        b = None if bias is None else bias[g * co:(g + 1) * co]
        outs.append(F.conv2d(x[:, g * ci:(g + 1) * ci], w[g * co:(g + 1) * co], b, stride=stride, padding=pad))
    return torch.cat(outs, 1)


def grouped_backward_by_slabs(dy, w, groups, pad, in_hw):
    """Its stride-1 backward-data pass: per group a dense convolution of the gradient slab with the flipped kernel, input and output channels
    swapped, padding k - 1 - p -- the pack weights.hip builds per group."""
    co = w.shape[0] // groups
    kh, kw = w.shape[2:]
    outs = []
    for g in range(groups):
        wf = w[g * co:(g + 1) * co].flip(2, 3).transpose(0, 1)
        outs.append(F.conv2d(F.pad(dy[:, g * co:(g + 1) * co], (kw - 1 - pad, kw - 1 - pad, kh - 1 - pad, kh - 1 - pad)), wf))
    out = torch.cat(outs, 1)
    assert tuple(out.shape[2:]) == tuple(in_hw)
    return out
