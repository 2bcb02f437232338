"""A catalogue of small layer programs around a depthwise convolution (a grouped launch with one input or one output channel per group:
xfr_amd/csrc/conv_depthwise.hip, configuration 14), one net per boundary of that kernel: a map of more than one tile, several images of a channel
in one tile, halos as large as the map, a kernel larger than the map, the global depthwise head, strided layers (the forward stride and the four
backward phases), rows and columns no output reaches, K = 1, channel multipliers, a bias, a batch prefix -- and a Ci = Co = 2 layer that the kernel
must leave to configuration 13.

The case class, the single-layer net and the tape builder are tests/grouped_nets.py's: every net is a dense 3x3 + BatchNorm + ReLU, the depthwise
layer + BatchNorm + ReLU, a Linear head.  A tile of the kernel is 1024 consecutive outputs of one channel, whole rows wide: dw_tiles (37 x 41 = 1517
outputs an image) has tile borders inside an image and in the middle of a row, so the halo of a tile comes from neighbouring pixels above, below
and beside the border, not from padding; there is no tiling along W to outgrow."""
from grouped_nets import GroupedCase, _single


def _mbv1_mini(p):
    """The head of a MobileNetV1 on 3 x 33 x 29: stem 3x3 s2 -> 8 (17 x 15), depthwise 3x3 s1, pointwise -> 16, depthwise 3x3 s2 (-> 9 x 8), pointwise
    -> 32, each with BatchNorm + ReLU, a Linear head on 9 x 8."""
    t = p.conv(0, 'conv1', 8, 3, stride=2, pad=1, bias=False)
    t = p.relu_(p.batchnorm(t, 'bn1'))
    t = p.conv(t, 'dw1', 8, 3, stride=1, pad=1, bias=False, groups=8)
    t = p.relu_(p.batchnorm(t, 'dw1_bn'))
    t = p.conv(t, 'pw1', 16, 1, bias=False)
    t = p.relu_(p.batchnorm(t, 'pw1_bn'))
    t = p.conv(t, 'dw2', 16, 3, stride=2, pad=1, bias=False, groups=16)
    t = p.relu_(p.batchnorm(t, 'dw2_bn'))
    t = p.conv(t, 'pw2', 32, 1, bias=False)
    t = p.relu_(p.batchnorm(t, 'pw2_bn'))
    return p.mark('classify', p.linear(t, 'fc', 5, (9, 8)))


def _dw(name, shape, k, s, p, target, seed, mult=1, bias=False, batch=None, groups=None):
    c, h, w = shape
    groups = groups or c
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    return GroupedCase(name, shape, _single(c, c * mult, groups, k, s, p, (oh, ow), bias=bias), target, seed, ('gconv', h, w, c, c * mult, groups, k, s, p), batch=batch)


CASES = [
    _dw('dw_tiles', (8, 37, 41), 3, 1, 1, 'a map of more than one tile, the tile borders inside a row; W % 4 != 0', 61),
    _dw('dw_7x7map', (16, 7, 7), 3, 1, 1, 'several images of a channel in one tile, no halo across an image boundary', 62, batch=3),
    _dw('dw5_p2', (12, 6, 5), 5, 1, 2, '25 taps, a halo comparable to the map', 63),
    _dw('dw7_p3', (12, 5, 4), 7, 1, 3, 'a kernel larger than the map, backward padding 3', 64),
    _dw('gdc7', (16, 7, 7), 7, 1, 0, 'the global depthwise head: M = NB forward, a full convolution from a 1 x 1 map backward', 65),
    _dw('dw3_s2_odd', (16, 13, 9), 3, 2, 1, 'strided forward, four phases scattered into a zero-filled target', 66),
    _dw('dw3_s2_p0', (16, 12, 10), 3, 2, 0, 'row 11 and column 9 of the input are reached by no output', 67),
    _dw('dw1_s2', (16, 13, 9), 1, 2, 0, 'K = 1, the scattered accumulate store', 68),
    _dw('mult3', (8, 10, 7), 3, 1, 1, 'Ci 1, Co 3 forward; Ci 3, Co 1, K 27 backward', 69, mult=3),
    _dw('mult3_s2', (8, 11, 9), 3, 2, 1, 'multiplier 3 by phases: K 12 / 6 / 6 / 3', 70, mult=3),
    _dw('dw_bias', (20, 9, 12), 3, 1, 1, 'bias and bias_pos; W % 4 == 0, the 16-byte path', 71, bias=True),
    _dw('dw_prefix', (16, 15, 13), 3, 1, 1, 'batch 3 on an engine of max_batch 8: in_nb > NB', 72, batch=3),
    _dw('pair_g', (16, 9, 8), 3, 1, 1, 'Ci = Co = 2: not a depthwise launch, stays on configuration 13', 73, groups=8),
    GroupedCase('mbv1_mini', (3, 33, 29), _mbv1_mini, 'stem, depthwise s1, pointwise, depthwise s2, pointwise, Linear', 74, ('dw2', 17, 15, 16, 16, 16, 3, 2, 1)),
]
BY_NAME = {c.name: c for c in CASES}
# the layers of a case that are depthwise launches: (weight prefix, H, W, channels in, channels out, groups, kernel, stride, pad)
DEPTHWISE_LAYERS = {c.name: [c.grouped] for c in CASES if c.name != 'pair_g'}
DEPTHWISE_LAYERS['mbv1_mini'] = [('dw1', 17, 15, 8, 8, 8, 3, 1, 1), ('dw2', 17, 15, 16, 16, 16, 3, 2, 1)]
