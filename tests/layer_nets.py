"""A catalogue of small layer programs, each built to cross one launch-form boundary of the engine at odd, non-square shapes.

Every entry is written once, against the `Program` builder's signature (xfr_amd/program.py); `NetCase.program()` runs that forward
on a real `Program`, `NetCase.tape()` runs the same forward on the CPU oracle's `Tape` (oracle/ebp_oracle.py) in float32 or float64.
Weights are seeded; every BatchNorm's running statistics are the per-channel mean / variance of its input over a calibration batch
(the float64 tape, layer by layer), so that activations stay O(1) through the whole net whatever its depth.

`target` names the launch form the net exists for; tests/test_layer_plan.py holds the planner to it.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ebp_oracle as O
from xfr_amd.program import Program


class _TapeBuilder(object):
    """The `Program` builder's signature over an oracle Tape: the same forward function drives both."""

    def __init__(self, tape, x, calibrate=None):
        self.t = tape
        self.x = x
        self.calibrate = calibrate          # dict to receive BatchNorm running statistics (calibration pass), else None
        self.marks = {}
        tape.pool_args = {}                 # max-pool output tensor -> (kernel, stride, pad, ceil_mode), for pool_windows_clear

    def conv(self, x, prefix, cout, k, stride=1, pad=0, bias=True, groups=1):
        return self.t.conv(x, prefix, stride=stride, pad=pad, groups=groups)

    def batchnorm(self, x, prefix, eps=1e-5):
        if self.calibrate is not None:
            v = self.t.T[x]
            mean = v.mean(dim=(0, 2, 3))
            var = v.var(dim=(0, 2, 3), unbiased=False)
            for name, val in ((prefix + '.running_mean', mean), (prefix + '.running_var', var)):
                self.calibrate[name] = val.float()
                self.t.p[name] = val.float().to(self.t.dtype)
        return self.t.batchnorm(x, prefix, eps)

    def relu_(self, x):
        return self.t.relu_(x)

    def maxpool(self, x, k, stride, pad=0, ceil_mode=False):
        out = self.t.maxpool(x, k, stride, pad, ceil_mode)
        self.t.pool_args[out] = (k, stride, pad, bool(ceil_mode))
        return out

    def avgpool(self, x, k, stride):
        return self.t.avgpool(x, k, stride)

    def add(self, a, b):
        return self.t.add(a, b)

    def concat_channels(self, x, channels):
        return self.t.concat_channels(x, channels)

    def multiply(self, x, n):
        return self.t.multiply(x, n)

    def linear(self, x, prefix, cout, in_hw, bias=True):
        # Program.linear reads its (C, H, W) input tensor directly -- no view between them -- so its hook shares that tensor with an in-place
        # ReLU's and fires after it (registration order): the flatten is part of the hooked call here, not a glue tensor of its own
        t = self.t

        def fn(ins, positive):
            return F.linear(ins[0].flatten(1), t._w(prefix + '.weight', positive), t._b(prefix + '.bias', positive))
        return t._record('Linear', [x], True, fn)

    def split(self, x):
        return self.t.split(x)

    def g_add(self, a, b):
        return self.t.g_add(a, b)

    def g_maxhalves(self, x):
        return self.t.g_max_halves(x)

    def g_normalize(self, x):
        return self.t.g_normalize(x)

    def mark(self, name, tensor):
        self.marks[name] = tensor
        return tensor


# ---- the forwards ------------------------------------------------------------------------------------------------------------------
def _stem(p):
    """7x7 s2 p3 on three channels (the tap4 stem; its image hook is the P[-1] gather) at 37 x 29 -> 19 x 15, max-pool 3/2/1 at odd
    sizes -> 10 x 8, a 3x3 64 -> 40 (ragged Cout), a Linear head."""
    t = p.conv(0, 'conv1', 64, 7, stride=2, pad=3, bias=False)
    t = p.relu_(p.batchnorm(t, 'bn1'))
    t = p.maxpool(t, 3, 2, 1)
    t = p.conv(t, 'conv2', 40, 3, stride=1, pad=1, bias=False)
    t = p.relu_(p.batchnorm(t, 'bn2'))
    return p.mark('classify', p.linear(t, 'fc', 5, (10, 8)))


def _projection(p):
    """A stage-opening ResNet-50 block with a 1x1 s2 projection shortcut on a 15 x 13 map (-> 8 x 7: the stride-2 scatter onto an odd map),
    main path 1x1 s2 -> 3x3 -> 1x1, functional add, ReLU."""
    t = p.conv(0, 'conv1', 64, 3, stride=1, pad=1, bias=False)
    t = p.relu_(p.batchnorm(t, 'bn1'))
    o = p.conv(t, 'b.reduce', 32, 1, stride=2, bias=False)
    o = p.relu_(p.batchnorm(o, 'b.reduce_bn'))
    o = p.conv(o, 'b.3x3', 32, 3, stride=1, pad=1, bias=False)
    o = p.relu_(p.batchnorm(o, 'b.3x3_bn'))
    o = p.conv(o, 'b.increase', 128, 1, bias=False)
    o = p.batchnorm(o, 'b.increase_bn')
    sc = p.conv(t, 'b.proj', 128, 1, stride=2, bias=False)
    sc = p.batchnorm(sc, 'b.proj_bn')
    t = p.relu_(p.g_add(sc, o))
    return p.mark('classify', p.linear(t, 'fc', 5, (8, 7)))


def _bf16x6(p):
    """3x3 128 -> 128 layers (K = 1152: covered by the bf16x6 kernel, staged as a patch) around a residual add at 15 x 17 (ragged M), then
    a 1x1 128 -> 256 -> 128 pair (K = 256 on the second: the shallowest 1x1 the bf16x6 kernel takes)."""
    t = p.conv(0, 'conv1', 128, 3, stride=1, pad=1, bias=False)
    r = p.relu_(p.batchnorm(t, 'bn1'))
    o = p.conv(r, 'conv2', 128, 3, stride=1, pad=1, bias=False)
    o = p.relu_(p.batchnorm(o, 'bn2'))
    o = p.conv(o, 'conv3', 128, 3, stride=1, pad=1, bias=False)
    o = p.batchnorm(o, 'bn3')
    t = p.relu_(p.add(o, r))
    t = p.conv(t, 'conv4', 256, 1, bias=False)
    t = p.relu_(p.batchnorm(t, 'bn4'))
    t = p.conv(t, 'conv5', 128, 1, bias=False)
    t = p.relu_(p.batchnorm(t, 'bn5'))
    return p.mark('classify', p.linear(t, 'fc', 5, (15, 17)))


def _halo(w):
    def fwd(p):
        """Two "same" 3x3 128 -> 128 layers on rows of %d: halo pad * W + pad = %d (the bf16x6 patch takes at most 64)."""
        t = p.conv(0, 'conv1', 128, 3, stride=1, pad=1, bias=False)
        t = p.relu_(p.batchnorm(t, 'bn1'))
        t = p.conv(t, 'conv2', 128, 3, stride=1, pad=1, bias=False)
        t = p.relu_(p.batchnorm(t, 'bn2'))
        return p.mark('classify', p.linear(t, 'fc', 5, (9, w)))
    fwd.__doc__ = fwd.__doc__ % (w, w + 1)
    return fwd


def _classifier(p):
    """A 512 x 4 x 5 map into a Linear 10240 -> 1037: very deep K over a few tiles (K-parts), ragged Cout, forward and backward."""
    t = p.conv(0, 'conv1', 512, 1, bias=False)
    t = p.relu_(p.batchnorm(t, 'bn1'))
    return p.mark('classify', p.linear(t, 'fc', 1037, (4, 5)))


def _valid_wide(p):
    """24 channels (Cin % 16 != 0: ci-major K), a 'valid' 5x5 (11 -> 7, backward padding 4) and a 3x3 pad 2 that grows the map (7 -> 9):
    the backward padding k - 1 - p is 0 there."""
    t = p.conv(0, 'conv0', 24, 3, stride=1, pad=1, bias=False)
    t = p.relu_(p.batchnorm(t, 'bn0'))
    t = p.conv(t, 'conv1', 32, 5, stride=1, pad=0, bias=True)
    t = p.relu_(p.batchnorm(t, 'bn1'))
    t = p.conv(t, 'conv2', 16, 3, stride=1, pad=2, bias=True)
    t = p.relu_(p.batchnorm(t, 'bn2'))
    return p.mark('classify', p.linear(t, 'fc', 5, (9, 9)))


def _strided(p):
    """A 1x1 stride-3 convolution (10 x 7 -> 4 x 3): the stride-s scatter of its backward-data GEMM (M = 70 n on the input side, 12 n on
    the output side)."""
    t = p.conv(0, 'conv0', 32, 3, stride=1, pad=1, bias=False)
    t = p.relu_(p.batchnorm(t, 'bn0'))
    t = p.conv(t, 'conv1', 48, 1, stride=3, bias=True)
    t = p.relu_(p.batchnorm(t, 'bn1'))
    return p.mark('classify', p.linear(t, 'fc', 5, (4, 3)))


def _stem_pool(pad, ceil_mode, hw):
    def fwd(p):
        """The ResNet stems on a map with W = 2 OW, W %% 8 == 0 (the row-pair max-pool kernels): 7x7 s2 p3 on three channels, max-pool 3/2/%d%s
        -> %d x %d, a 3x3 64 -> 40, a Linear head."""
        t = p.conv(0, 'conv1', 64, 7, stride=2, pad=3, bias=False)
        t = p.relu_(p.batchnorm(t, 'bn1'))
        t = p.maxpool(t, 3, 2, pad, ceil_mode=ceil_mode)
        t = p.conv(t, 'conv2', 40, 3, stride=1, pad=1, bias=False)
        t = p.relu_(p.batchnorm(t, 'bn2'))
        return p.mark('classify', p.linear(t, 'fc', 5, hw))
    fwd.__doc__ = fwd.__doc__ % ((pad, ' ceil_mode' if ceil_mode else '') + tuple(hw))
    return fwd


def _pooled(pool, k, stride, hw):
    def fwd(p):
        """conv3x3 32, BN, ReLU, a %s-pool %d/%d without padding -> %d x %d, conv3x3 16, BN, ReLU, a Linear head."""
        t = p.conv(0, 'conv1', 32, 3, stride=1, pad=1, bias=False)
        t = p.relu_(p.batchnorm(t, 'bn1'))
        t = p.maxpool(t, k, stride) if pool == 'max' else p.avgpool(t, k, stride)
        t = p.conv(t, 'conv2', 16, 3, stride=1, pad=1, bias=False)
        t = p.relu_(p.batchnorm(t, 'bn2'))
        return p.mark('classify', p.linear(t, 'fc', 5, hw))
    fwd.__doc__ = fwd.__doc__ % ((pool, k, stride) + tuple(hw))
    return fwd


def _mfm(hw):
    def fwd(p):
        """Light-CNN's direct stem (5x5, one channel, pad 2) with MaxFeatureMap 16 -> 8, the pool pair max + avg (odd sizes floor) -> %d x %d,
        a MaxFeatureMap 3x3 (co_pair rows), a Linear head."""
        t = p.g_maxhalves(p.split(p.conv(0, 'conv1', 16, 5, stride=1, pad=2)))
        t = p.g_add(p.maxpool(t, 2, 2), p.avgpool(t, 2, 2))
        t = p.g_maxhalves(p.split(p.conv(t, 'conv2', 16, 3, stride=1, pad=1)))
        return p.mark('classify', p.linear(t, 'fc', 5, hw))
    fwd.__doc__ = fwd.__doc__ % tuple(hw)
    return fwd


def _avg_shortcut(hw):
    def fwd(p):
        """An STR-ResNet down-sampling block (AvgPool2d(2) + ConcatChannels shortcut, resnet.py:210-213) -> %d x %d."""
        t = p.conv(0, 'conv1', 64, 3, stride=1, pad=1, bias=False)
        t = p.relu_(p.batchnorm(t, 'bn1'))
        o = p.conv(t, 'b.conv1', 32, 1, stride=2, bias=False)
        o = p.relu_(p.batchnorm(o, 'b.bn1'))
        o = p.conv(o, 'b.conv2', 32, 3, stride=1, pad=1, bias=False)
        o = p.relu_(p.batchnorm(o, 'b.bn2'))
        o = p.conv(o, 'b.conv3', 128, 1, bias=False)
        o = p.batchnorm(o, 'b.bn3')
        r = p.concat_channels(p.avgpool(t, 2, 2), 1)
        t = p.relu_(p.add(o, r))
        return p.mark('classify', p.linear(t, 'fc', 5, hw))
    fwd.__doc__ = fwd.__doc__ % tuple(hw)
    return fwd


def _global_tail(cout, k, normalize, relu=True):
    def fwd(p):
        """conv3x3 %d, BN%s, a global average pool %d x %d%s, a Linear head on the 1 x 1 map."""
        t = p.conv(0, 'conv1', cout, 3, stride=1, pad=1, bias=False)
        t = p.batchnorm(t, 'bn1')
        if relu:
            t = p.relu_(t)
        t = p.avgpool(t, k, k)
        if normalize:
            t = p.multiply(p.g_normalize(t), 50.0)
        return p.mark('classify', p.linear(t, 'fc', 5, (1, 1)))
    fwd.__doc__ = fwd.__doc__ % (cout, ', ReLU' if relu else ' (no ReLU: the pooled map is signed)', k, k,
                                 ', the STR-ResNet encode tail F.normalize and Multiply(50)' if normalize else '')
    return fwd


class NetCase(object):
    def __init__(self, name, in_shape, forward, target, seed):
        self.name = name
        self.in_shape = tuple(in_shape)
        self.forward = forward
        self.target = target
        self.seed = seed
        self._params = None

    def program(self):
        prog = Program(self.in_shape)
        self.forward(prog)
        return prog

    @property
    def seed_tensor(self):
        return self.program().marks['classify']

    def inputs(self, n, seed=0):
        g = torch.Generator().manual_seed(1000 * self.seed + 17 + seed)
        return torch.randn((n,) + self.in_shape, generator=g)

    def params(self):
        """Seeded weights (fan-in scaled; a grouped convolution's are (cout, Cin / groups, kh, kw) -- Program keeps `groups` in the op's ceil_mode
        slot), BatchNorm affine parameters around one, running statistics from a calibration batch."""
        if self._params is not None:
            return self._params
        prog = self.program()
        g = torch.Generator().manual_seed(7919 * self.seed + 3)
        ch = prog.tensor_channels()
        sd = {}
        for o in prog.ops:
            names = prog.weight_names
            if o.w_weight < 0:
                continue
            wname = names[o.w_weight]
            if o.kind in (1, 9):                              # CONV, LINEAR
                cin = ch[o.in0] // max(o.ceil_mode, 1) if o.kind == 1 else ch[o.in0]
                fan = cin * o.kh * o.kw
                shape = (o.cout, cin, o.kh, o.kw) if o.kind == 1 else (o.cout, fan)
                sd[wname] = torch.randn(shape, generator=g) * (1.5 / np.sqrt(fan))
                if o.w_bias >= 0:
                    sd[names[o.w_bias]] = 0.1 * torch.randn((o.cout,), generator=g)
            elif o.kind == 2:                                 # BATCHNORM
                c = ch[o.in0]
                sd[wname] = 0.5 + torch.rand((c,), generator=g)
                sd[names[o.w_bias]] = 0.2 * torch.randn((c,), generator=g)
                sd[names[o.w_mean]] = torch.zeros((c,))
                sd[names[o.w_var]] = torch.ones((c,))
        calib = {}
        tape = O.Tape(sd, dtype=torch.float64)
        b = _TapeBuilder(tape, None, calibrate=calib)
        tape.input(self.inputs(4, seed=99))
        self.forward(b)
        sd.update(calib)
        self._params = sd
        return sd

    def tape(self, x, dtype=torch.float32, params=None):
        """The forward on the oracle tape -> (tape, output tensor id); `params` replaces the case's own (a test that edits one)."""
        tape = O.Tape(self.params() if params is None else params, dtype=dtype)
        b = _TapeBuilder(tape, x)
        tape.input(x)
        return tape, self.forward(b)

    def oracle_P(self, x, seed, mode, dtype=torch.float32):
        """Whitebox.P of one sweep (firing order, the image hook last) on the tape in `dtype`."""
        tape, out = self.tape(x, dtype)
        P, names = tape.backward(out, seed, mode, 1e-16)
        return P, names, tape


CASES = [
    NetCase('stem', (3, 37, 29), _stem, 'tap4 stem, P[-1] gather at odd sizes, ragged Cout, max-pool edges', 1),
    NetCase('projection', (64, 15, 13), _projection, 'stride-2 scatter onto an odd map, projection side branch (fusion bit 7)', 2),
    NetCase('avg_shortcut', (64, 18, 14), _avg_shortcut((9, 7)), 'compact as_strided + EW_AVGUP_IN (fusion bit 6)', 3),
    NetCase('bf16x6', (128, 15, 17), _bf16x6, 'patch staging, ragged M, forward and backward bf16x6', 4),
    NetCase('halo64', (128, 9, 63), _halo(63), 'halo 64: the bf16x6 patch', 5),
    NetCase('halo65', (128, 9, 64), _halo(64), 'halo 65: the bf16x6 slab', 6),
    NetCase('mfm', (1, 37, 31), _mfm((18, 15)), 'co_pair rows and EW_MAXHALF_IN at odd sizes (W % 4 != 0: no direct stem, no pool-pair fusion): the scalar pools and their separate VJPs', 7),
    NetCase('classifier', (512, 4, 5), _classifier, 'deep-K K-parts over few tiles, ragged Cout', 8),
    NetCase('valid_wide', (24, 11, 11), _valid_wide, 'Cin % 16 != 0 (ci-major K), backward padding k - 1 - p = 0', 9),
    NetCase('strided', (32, 10, 7), _strided, 'stride-3 1x1 scatter, M % 4 != 0', 10),
    # the float4 / row-pair / fused forms of the pooling and tail kernels (xfr_amd/csrc/elementwise.hip), at the smallest shapes that reach them
    NetCase('stem_rows', (3, 25, 32), _stem_pool(1, False, (7, 8)), 'maxpool_fwd_rows<3,1> (left column in and out, last window row clipped), maxpool_bwd_v4<3,2>', 11),
    NetCase('ceil_rows', (3, 23, 32), _stem_pool(0, True, (6, 8)), 'maxpool_fwd_rows<3,0> under ceil_mode (right column in and out, bottom row out of range)', 20),      # (seed 12 leaves near-tie windows: pool_windows_clear)
    NetCase('pool_generic', (16, 12, 12), _pooled('max', 3, 3, (4, 4)), 'maxpool_fwd_v4<0,0>, maxpool_bwd_v4<0,0>', 13),
    NetCase('pool_odd17', (8, 10, 17), _pooled('max', 2, 2, (5, 8)), 'maxpool_fwd_v4<2,2> without the row-pair form (W = 2 OW + 1), scalar VJP', 14),
    NetCase('mfm_pool2', (1, 20, 24), _mfm((10, 12)), 'stem5_mfm, pool2_fwd, float4 EW_POOL2_IN; un-fused: rows<2,0> and the 2/2 float4 pools and VJPs', 15),
    NetCase('avg_shortcut_v4', (64, 16, 24), _avg_shortcut((8, 12)), 'avgpool_fwd_v4<2,2> with zero planes, float4 EW_AVGUP_IN; un-fused: avgpool_bwd_v4<2,2>', 16),
    NetCase('encode_tail', (32, 5, 5), _global_tail(80, 5, True), 'global average pool (partial last block of 128 planes) and its VJP, normalize forward / VJP, Multiply', 17),
    NetCase('global_big', (16, 12, 12), _global_tail(48, 12, False), 'a global pool whose 128 planes outgrow 64 KB of LDS: generic forward, global VJP', 18),
    NetCase('avg_generic', (16, 12, 12), _pooled('avg', 3, 3, (4, 4)), 'avgpool_fwd_v4<0,0>, avgpool_bwd_v4<0,0>', 19),
    NetCase('signed_tail', (32, 5, 5), _global_tail(80, 5, False, relu=False), 'the global average pool of a signed map: its positive pass clamps the input (relu_in = 1), partial last block of 128 planes', 21),
]
BY_NAME = {c.name: c for c in CASES}

# The kernel variants each net must launch, keyed by where.  The names are those of xfr_elementwise_variant_name.
# 'firing' means during test_gpu_layer_parity.test_every_firing_matches_float64, whose observing sweeps run with the default fusion.
# A schedule tag means during that entry of the schedule matrix.
# 'all' stands for 'firing', 'fusion0' and 'fusion_separate'.  It does not apply under the 'default' tag: see required_variants.
# A variant that the default schedule must launch as well is therefore named under 'default' again, as in avg_shortcut_v4.
# No counter separates relu_in = 1 from relu_in = 0 launches.  That signed_tail takes the clamped path of the global pool is proven by its
# values: the float64 comparison fails without the clamp.
_UNFUSED_PAIR = ['maxpool_fwd_rows<2,0>', 'avgpool_fwd_v4<2,2>', 'maxpool_bwd_v4<2,2>', 'avgpool_bwd_v4<2,2>']
REQUIRED_VARIANTS = {
    'stem': {'firing': ['maxpool_fwd_v4<3,2>', 'maxpool_bwd']},
    'mfm': {'firing': ['maxpool_fwd', 'avgpool_fwd', 'maxpool_bwd', 'avgpool_bwd']},
    'avg_shortcut': {'firing': ['avgpool_fwd']},
    'stem_rows': {'all': ['maxpool_fwd_rows<3,1>', 'maxpool_bwd_v4<3,2>']},
    'ceil_rows': {'all': ['maxpool_fwd_rows<3,0>', 'maxpool_bwd_v4<3,2>']},
    'pool_generic': {'all': ['maxpool_fwd_v4<0,0>', 'maxpool_bwd_v4<0,0>']},
    'pool_odd17': {'all': ['maxpool_fwd_v4<2,2>', 'maxpool_bwd']},
    'mfm_pool2': {'firing': ['stem5_mfm', 'pool2_fwd', 'ew_chain_v4/pool2_in'], 'default': ['stem5_mfm', 'pool2_fwd', 'ew_chain_v4/pool2_in'],
                  'fusion0': _UNFUSED_PAIR, 'fusion_separate': _UNFUSED_PAIR},
    'avg_shortcut_v4': {'all': ['avgpool_fwd_v4<2,2>'], 'default': ['avgpool_fwd_v4<2,2>', 'ew_chain_v4/avgup_in'],
                        'fusion0': ['avgpool_bwd_v4<2,2>'], 'fusion_separate': ['avgpool_bwd_v4<2,2>']},
    'encode_tail': {'all': ['avgpool_global_fwd', 'avgpool_global_bwd', 'normalize_fwd', 'normalize_bwd']},
    'global_big': {'all': ['avgpool_fwd', 'avgpool_global_bwd']},
    'avg_generic': {'all': ['avgpool_fwd_v4<0,0>', 'avgpool_bwd_v4<0,0>']},
    'signed_tail': {'all': ['avgpool_global_fwd', 'avgpool_global_bwd']},
}


def required_variants(name, where):
    """Sorted names of the variants net `name` must launch during `where`."""
    r = REQUIRED_VARIANTS.get(name, {})
    return sorted(set(r.get(where, [])) | set(r.get('all', []) if where in ('firing', 'fusion0', 'fusion_separate') else []))


def pool_window_columns(v, k, s, p, out_hw):
    """The max-pool windows of v (N x C x H x W) as columns, N x C x (k k) x (OH OW), padding as -inf.  out_hw is the pool's output size: under
    ceil_mode the window grid reaches past the right / bottom edge, and what lies there is padding like the rest."""
    eb = max((out_hw[0] - 1) * s + k - (v.shape[2] + 2 * p), 0)
    er = max((out_hw[1] - 1) * s + k - (v.shape[3] + 2 * p), 0)
    cols = F.unfold(F.pad(v, (p, p + er, p, p + eb), value=float('-inf')), k, stride=s)        # N x (C k k) x L
    return cols.view(v.shape[0], v.shape[1], k * k, -1)


def pool_windows_clear(tape64, rel_gap=1e-6):
    """Every max-pool window of the float64 forward has a unique maximum by a margin of rel_gap x max|input| (or an exact tie, which the
    first-index rule decides), and every MaxFeatureMap pair is ordered by that margin: no argmax can flip between two float32 implementations.
    -> list of (call, offending elements)."""
    bad = []
    for c in tape64.calls:
        v = tape64.T[c.ins[0]]
        scale = float(v.abs().max())
        if c.name == 'MaxPool2d':
            k, s, p, _ = tape64.pool_args[c.out]            # ceil_mode shows in the output's shape, which sets the window grid
            cols = pool_window_columns(v, k, s, p, tape64.T[c.out].shape[2:])
            top2 = cols.topk(2, dim=2).values
            gap = top2[:, :, 0] - top2[:, :, 1]
            assert gap.numel() == tape64.T[c.out].numel()
            near = (gap > 0) & (gap < rel_gap * scale)
        elif c.name == 'max':
            a, b = torch.split(v, v.shape[1] // 2, 1)
            d = (a - b).abs()
            near = (d > 0) & (d < rel_gap * scale)
        else:
            continue
        if bool(near.any()):
            bad.append((c.name, int(near.sum())))
    return bad


def phases(H, W, k_channels, k, s, p):
    """The phase launches of a k x k / stride s / pad p convolution's backward-data pass onto an H x W map by the formulas of the phase form
    (xfr_amd/csrc/plan.hip PhaseRec), k_channels GEMM rows per tap (cout; of ONE group for a grouped layer)
    -> list of dicts (r, c, ka, kb, K, ih0, iw0, nq, nu)."""
    out = []
    for r in range(min(s, k)):
        for c in range(min(s, k)):
            ka, kb = -(-(k - r) // s), -(-(k - c) // s)
            q0, u0 = max(0, -(-(p - r) // s)), max(0, -(-(p - c) // s))
            ih0, iw0 = s * q0 + r - p, s * u0 + c - p
            if ih0 >= H or iw0 >= W:
                continue
            out.append(dict(r=r, c=c, ka=ka, kb=kb, K=k_channels * ka * kb, ih0=ih0, iw0=iw0, nq=(H - 1 - ih0) // s + 1, nu=(W - 1 - iw0) // s + 1))
    return out
