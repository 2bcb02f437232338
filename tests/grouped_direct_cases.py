"""The single launches tests/test_gpu_grouped_direct.py puts through xfr_debug_conv_grouped: the smallest shapes that take each branch of
xfr_amd/csrc/conv_depthwise.hip (configuration 14) and xfr_amd/csrc/conv_group.hip (configuration 13) that the layer catalogues (depthwise_nets.py,
grouped_nets.py) do not reach, the inputs of every launch (fixed seeds) and its float64 reference.  A plain module: no test in it, no device, no library.

A case is ONE launch as the kernels see it: Ci and Co are the channels of one group, (H, W) the map the launch reads.  role says where the engine makes
such a launch: 'fwd' a forward layer, 'bwd' the backward-data pass of the stride-1 layer `layer` (the launch reads dY with the flipped, transposed
weight and padding k - 1 - p), 'phase' one phase of the backward-data pass of the strided layer `layer`, 'plain' a launch stated by its geometry only.
tests/test_grouped_direct_cases.py proves on the CPU that the 'bwd' and 'phase' launches, through `reference`, are torch autograd's input gradient.

expect = (cfg, TM): the configuration a cfg-0 call runs and the depthwise launcher's tile (0 on configuration 13).  The TM values are stated here and
restated from the launcher's sizing loop by `launcher_tile`; the GPU file asserts what the library reports.
"""
import torch
import torch.nn.functional as F

CFG_GROUP, CFG_DEPTHWISE = 13, 14
X_FLOATS, SPAN_MAX, MAX_CH, MAX_TAP = 13312, 1 << 22, 8, 7      # conv_depthwise.hip's LDS budget for X, span cap, channel cap, tap cap
MARGIN = 64                                                    # floats in front of and behind every device tensor (a multiple of 4: alignment is the case's)


class Case(object):
    def __init__(self, name, G, Ci, Co, NB, H, W, kh, kw=None, stride=1, pad=0, pad_dw=0, relu_in=0, nhalves=1, accumulate=0, in_nb=None, out_nb=None,
                 out_stride=1, target=None, origin=(0, 0), bias=False, in_shift=0, out_shift=0, expect=(CFG_DEPTHWISE, 1024), role='fwd', layer=None,
                 K=None, M=None, what=''):
        self.name, self.G, self.Ci, self.Co, self.NB, self.H, self.W = name, G, Ci, Co, NB, H, W
        self.kh, self.kw, self.stride, self.pad, self.pad_dw = kh, kh if kw is None else kw, stride, pad, pad_dw
        self.relu_in, self.nhalves, self.accumulate = relu_in, nhalves, accumulate
        self.in_nb, self.out_nb = in_nb or NB, out_nb or NB
        self.OH = (H + 2 * pad - self.kh) // stride + 1
        self.OW = (W + 2 * (pad + pad_dw) - self.kw) // stride + 1
        self.out_stride, self.target, self.origin = out_stride, target or (self.OH, self.OW), origin
        self.dense = target is None
        self.bias, self.in_shift, self.out_shift = bias, in_shift, out_shift
        self.expect, self.role, self.layer, self.K, self.M, self.what = expect, role, layer, K, M, what
        self.cin, self.cout = G * Ci, G * Co
        self.seed = 1000 + sum(ord(c) * (i + 1) for i, c in enumerate(name))

    @property
    def eligible(self):
        """A cfg-14 call launches (the depthwise kernel takes it)."""
        return self.expect[0] == CFG_DEPTHWISE


def launcher_tile(c):
    """launch_conv_depthwise's caps and sizing loop, restated: the TM it launches with, or 0 where it returns false."""
    if (c.Ci != 1 and c.Co != 1) or max(c.Ci, c.Co) > MAX_CH or c.kh > MAX_TAP or c.kw > MAX_TAP:
        return 0
    Wp = (c.OW - 1) * c.stride + c.kw
    tm = 1024
    while tm >= 128:
        R = min((tm - 1) // c.OW + 2, c.NB * c.OH)
        I = min(c.NB, (R + c.OH - 2) // c.OH + 1)
        rows = R * c.stride + I * max(c.kh - c.stride, 0)
        if c.Ci * rows * Wp <= X_FLOATS and (I + 1) * c.H * c.W < SPAN_MAX and c.OH * c.OW + tm < SPAN_MAX:
            return tm
        tm //= 2
    return 0


def _bwd(name, G, mult, NB, H, W, k, p, expect, K, M, what, **kw):
    """The backward-data launch of the stride-1 depthwise layer (channel multiplier `mult`, k x k, padding p) on an H x W map."""
    return Case(name, G, mult, 1, NB, H, W, k, pad=k - 1 - p, expect=expect, role='bwd', layer=dict(G=G, Ci=1, Co=mult, k=k, s=1, p=p, H=H, W=W), K=K, M=M,
                what=what, **kw)


def phase_geometry(H, W, k, s, p):
    """The phases of a k x k / stride s / padding p layer's backward-data pass onto an H x W map (plan.hip PhaseRec, bwd_conv_params)."""
    out = []
    for r in range(min(s, k)):
        for c in range(min(s, k)):
            ka, kb = -(-(k - r) // s), -(-(k - c) // s)
            q0, u0 = max(0, -(-(p - r) // s)), max(0, -(-(p - c) // s))
            ih0, iw0 = s * q0 + r - p, s * u0 + c - p
            if ih0 < H and iw0 < W:
                out.append(dict(r=r, c=c, ka=ka, kb=kb, q0=q0, u0=u0, ih0=ih0, iw0=iw0, nq=(H - 1 - ih0) // s + 1, nu=(W - 1 - iw0) // s + 1))
    return out


def phase_case(name, layer, NB, r, c, expect, what, K=None, M=None):
    """Phase (r, c) of `layer`'s backward-data pass as a launch: dY under the phase's flipped sub-kernel at stride 1, scattered with the layer's stride
    from (ih0, iw0) on, added to the target.  Only phases whose nq x nu is what the padding gives are a launch of the debug entry (it derives OH, OW)."""
    ph = [q for q in phase_geometry(layer['H'], layer['W'], layer['k'], layer['s'], layer['p']) if (q['r'], q['c']) == (r, c)][0]
    k, s, p = layer['k'], layer['s'], layer['p']
    dh, dw = (layer['H'] + 2 * p - k) // s + 1, (layer['W'] + 2 * p - k) // s + 1
    pad = ph['ka'] - 1 - ph['q0']
    cs = Case(name, layer['G'], layer['Co'], layer['Ci'], NB, dh, dw, ph['ka'], ph['kb'], pad=pad, pad_dw=(ph['kb'] - 1 - ph['u0']) - pad, accumulate=1,
              out_stride=s, target=(layer['H'], layer['W']), origin=(ph['ih0'], ph['iw0']), expect=expect, role='phase', layer=layer, K=K, M=M, what=what)
    assert (cs.OH, cs.OW) == (ph['nq'], ph['nu']), (name, cs.OH, cs.OW, ph)
    cs.phase = (r, c)
    return cs


_PH_VEC = dict(G=3, Ci=1, Co=2, k=3, s=2, p=1, H=11, W=17)
_PH_ODD = dict(G=3, Ci=1, Co=2, k=3, s=2, p=1, H=11, W=15)
D14 = CFG_DEPTHWISE

DEPTHWISE = [
    Case('vec_tiles', 4, 1, 1, 9, 12, 12, 3, pad=1, K=9, M=1296, what='two tiles, the border at image 7 row 1 column 4, VEC output, 16-byte staging'),
    Case('m1024', 3, 1, 1, 4, 16, 16, 3, pad=1, K=9, M=1024, what='M exactly one tile'),
    Case('m1025', 3, 1, 1, 1, 25, 41, 3, pad=1, relu_in=1, K=9, M=1025, what='one output in the second tile, scalar path'),
    Case('co2', 6, 1, 2, 2, 9, 8, 3, pad=1, nhalves=2, bias=True, K=9, M=144, what='CO 2, two halves'),
    Case('co5', 4, 1, 5, 2, 9, 8, 3, pad=1, nhalves=2, bias=True, relu_in=1, K=9, M=144, what='CO 8 with three dead columns'),
    Case('co8', 3, 1, 8, 2, 9, 8, 3, pad=1, nhalves=2, bias=True, K=9, M=144, what='CO 8 full: 64 accumulators a thread'),
    _bwd('ci8', 3, 8, 2, 9, 8, 3, 1, (D14, 1024), 72, 144, 'the backward role, Ci 8'),
    _bwd('tm512', 2, 8, 3, 50, 4, 7, 3, (D14, 512), 392, 600, 'TM 512, two tiles, VEC'),
    Case('tm512_batch', 2, 1, 1, 128, 5, 5, 7, stride=2, pad=3, expect=(D14, 512), K=49, M=1152, what='TM 512, three tiles of about 57 images: a tiny map at a large batch'),
    _bwd('tm256', 2, 8, 4, 4, 52, 7, 3, (D14, 256), 392, 832, 'TM 256, four tiles, VEC', relu_in=1),
    _bwd('tm256_odd', 2, 8, 3, 4, 50, 7, 3, (D14, 256), 392, 600, 'TM 256, scalar output and staging'),
    Case('tm128', 2, 8, 1, 3, 6, 48, 7, stride=2, pad=3, expect=(D14, 128), K=392, M=216, what='TM 128, two tiles, VEC'),
    Case('tm128_odd', 2, 8, 1, 3, 5, 45, 7, stride=2, pad=3, expect=(D14, 128), K=392, M=207, what='TM 128, scalar'),
    Case('no_tile', 2, 8, 1, 3, 4, 57, 7, stride=2, pad=3, expect=(CFG_GROUP, 0), K=392, M=174, what='no tile fits the LDS budget'),
    Case('cap_co9', 2, 1, 9, 2, 9, 8, 3, pad=1, expect=(CFG_GROUP, 0), K=9, M=144, what='Co above the cap'),
    Case('cap_ci9', 2, 9, 1, 2, 9, 8, 3, pad=1, expect=(CFG_GROUP, 0), K=81, M=144, what='Ci above the cap'),
    Case('cap_k8', 3, 1, 1, 2, 9, 8, 8, pad=3, expect=(CFG_GROUP, 0), K=64, M=112, what='8 x 8 taps'),
    Case('cap_pair', 3, 2, 2, 2, 9, 8, 3, pad=1, expect=(CFG_GROUP, 0), K=18, M=144, what='Ci = Co = 2: not depthwise'),
    Case('gdc', 8, 1, 1, 5, 7, 7, 7, K=49, M=5, what='M = NB = 5, OW 1, five images in one tile'),
    Case('k1_s2', 4, 1, 1, 2, 13, 9, 1, stride=2, K=1, M=70, what='stride above the kernel'),
    Case('k1_pad2', 4, 1, 1, 2, 5, 4, 1, pad=2, bias=True, K=1, M=144, what='outputs wholly in padding equal the bias'),
    Case('k7_on_3x2', 4, 1, 1, 2, 3, 2, 7, pad=3, K=49, M=12, what='kernel larger than the map'),
    Case('taps_3x5', 3, 1, 2, 2, 9, 8, 3, 5, pad=1, pad_dw=1, role='plain', K=15, M=144, what='pad_dw > 0'),
    Case('taps_5x3', 3, 2, 1, 2, 9, 8, 5, 3, pad=2, pad_dw=-1, role='plain', K=30, M=144, what='pad_dw < 0'),
    Case('scatter_vec', 3, 4, 1, 2, 6, 9, 2, accumulate=1, out_stride=2, target=(11, 16), origin=(1, 1), role='plain', K=16, M=80,
         what='the phase store from the VEC decode: OW 8, a target of (2 OH + 1) x (2 OW), out0 one row and one column in'),
    Case('scatter_odd', 3, 4, 1, 2, 6, 8, 2, accumulate=1, out_stride=2, target=(11, 14), origin=(1, 1), role='plain', K=16, M=70,
         what='the phase store from the scalar decode: OW 7'),
    phase_case('phase_vec', _PH_VEC, 2, 0, 0, (D14, 1024), 'phase (0, 0) of a 3x3 / s2 / p1 multiplier-2 layer on 11 x 17: OW 8, scattered from (1, 1)', K=8, M=80),
    phase_case('phase_odd', _PH_ODD, 2, 0, 0, (D14, 1024), 'the same on 11 x 15: OW 7', K=8, M=70),
    Case('prefix_odd', 4, 1, 1, 3, 15, 13, 3, pad=1, in_nb=8, out_nb=5, K=9, M=585, what='a batch prefix, scalar path'),
    Case('prefix_vec', 4, 1, 1, 3, 12, 12, 3, pad=1, in_nb=8, out_nb=5, K=9, M=432, what='a batch prefix, VEC path'),
    Case('in_off1', 4, 1, 1, 9, 12, 12, 3, pad=1, in_shift=1, K=9, M=1296, what='vec_tiles with `in` one float off alignment: scalar staging at W % 4 == 0'),
    Case('out_off1', 4, 1, 1, 9, 12, 12, 3, pad=1, out_shift=1, K=9, M=1296, what='vec_tiles with out0 one float off alignment: scalar stores from the VEC decode'),
    Case('acc_vec', 4, 1, 1, 9, 12, 12, 3, pad=1, accumulate=1, nhalves=2, bias=True, K=9, M=1296, what='read-add-store on the 16-byte path, two halves'),
]


def _grp(name, Ci, Co, k, role, K, what, NBs=(2, 3), H=5, W=7, layer=None, pad=None):
    pad = (1 if k == 3 else 0) if pad is None else pad
    return [Case('%s/nb%d' % (name, nb), 2, Ci, Co, nb, H, W, k, pad=pad, nhalves=2, bias=True, expect=(CFG_GROUP, 0), role=role, layer=layer, K=K,
                 M=nb * ((H + 2 * pad - k) + 1) * ((W + 2 * pad - k) + 1), what=what) for nb in NBs]


GROUPED = (
    _grp('rb4', 4, 64, 3, 'fwd', 36, 'RB 4: four row blocks, one chunk') +
    _grp('rb4_ragged', 4, 72, 3, 'fwd', 36, 'RB 4: five row blocks, two chunks, the second with three dead blocks and a ragged last block') +
    _grp('rb4_back', 72, 4, 3, 'bwd', 648, 'the backward role: K 648, 21 K chunks, the tap counters wrap across chunk borders',
         layer=dict(G=2, Ci=4, Co=72, k=3, s=1, p=1, H=5, W=7)) +
    _grp('rb2_k1', 4, 24, 1, 'fwd', 4, 'RB 2, 1x1: K 4, one K step') +
    _grp('m257', 4, 72, 3, 'fwd', 36, 'rb4_ragged at M 257: one column in the second workgroup, three dead waves there', NBs=(1,), H=1, W=257)
)
CASES = DEPTHWISE + GROUPED
BY_NAME = {c.name: c for c in CASES}
ISOLATION = ('co5', 'rb4_ragged/nb3')          # one case per kernel for the group-isolation check


def prepared_weight(w, G, stride=1, r=0, c=0):
    """The weight of the backward-data launch of a grouped layer with weight w [G Co][Ci][kh][kw]: the taps (r + stride i, c + stride j), flipped,
    input and output channels of every group swapped -> [G Ci][Co][ka][kb].  What weights.hip packs for the stride-1 pass (stride 1) and per phase."""
    Co, Ci = w.shape[0] // G, w.shape[1]
    sub = w[:, :, r::stride, c::stride].flip(2, 3)
    return sub.reshape(G, Co, Ci, sub.shape[2], sub.shape[3]).transpose(1, 2).reshape(G * Ci, Co, sub.shape[2], sub.shape[3]).contiguous()


def layer_weight(case):
    """The float32 weight [G Co][Ci][k][k] of the forward layer behind a 'bwd' or 'phase' case."""
    L = case.layer
    g = torch.Generator().manual_seed(case.seed + 1)
    return (torch.randn((L['G'] * L['Co'], L['Ci'], L['k'], L['k']), generator=g) / (L['Ci'] * L['k'] * L['k']) ** 0.5).float()


def inputs(case):
    """-> dict of float32 CPU tensors: x [cin][in_nb][H][W] (images nb .. in_nb - 1 NaN), w in torch layout, bias / bias_pos or None, and pre0 / pre1
    [cout][out_nb][target], the pattern the outputs hold before the launch."""
    g = torch.Generator().manual_seed(case.seed)
    x = torch.randn((case.cin, case.in_nb, case.H, case.W), generator=g)
    x[:, case.NB:] = float('nan')
    if case.role in ('bwd', 'phase'):
        r, c = getattr(case, 'phase', (0, 0))
        w = prepared_weight(layer_weight(case), case.G, case.layer['s'], r, c)
    else:
        w = torch.randn((case.cout, case.Ci, case.kh, case.kw), generator=g) / (case.Ci * case.kh * case.kw) ** 0.5
    assert tuple(w.shape) == (case.cout, case.Ci, case.kh, case.kw), (case.name, tuple(w.shape))
    bias = torch.randn(case.cout, generator=g) if case.bias else None
    bias_pos = bias.clamp(min=0) if case.bias and case.nhalves == 2 else None
    shape = (case.cout, case.out_nb) + tuple(case.target)
    pre0 = torch.rand(shape, generator=g) * 2 - 1
    pre1 = torch.rand(shape, generator=g) * 2 - 1
    return dict(x=x.float(), w=w.float().contiguous(), bias=bias, bias_pos=bias_pos, pre0=pre0.float(), pre1=pre1.float())


def live_view(case, out):
    """The elements of an output tensor [cout][out_nb][target] the launch writes: [cout][NB][OH][OW]."""
    (r0, c0), s = case.origin, case.out_stride
    return out[:, :case.NB, r0::s, c0::s][:, :, :case.OH, :case.OW]


def conv(case, x, w, bias, dtype):
    """The launch's arithmetic in `dtype`: [cout][NB][OH][OW]."""
    xn = x[:, :case.NB].permute(1, 0, 2, 3).to(dtype)
    if case.relu_in:
        xn = xn.clamp(min=0)
    pw = case.pad + case.pad_dw
    y = F.conv2d(F.pad(xn, (pw, pw, case.pad, case.pad)), w.to(dtype), None if bias is None else bias.to(dtype), stride=case.stride, groups=case.G)
    assert tuple(y.shape[2:]) == (case.OH, case.OW), (case.name, tuple(y.shape))
    return y.permute(1, 0, 2, 3)


def reference(case, inp, dtype=torch.float64):
    """(out0, out1) after the launch, in `dtype`: the pre-filled tensors with conv(...) placed (added where the launch accumulates) at the live
    elements; out1 is the untouched pattern for a one-half launch."""
    outs = []
    for half in range(2):
        out = inp['pre%d' % half].to(dtype).clone()
        if half < case.nhalves:
            w = inp['w'] if half == 0 else inp['w'].clamp(min=0)
            y = conv(case, inp['x'], w, inp['bias'] if half == 0 else inp['bias_pos'], dtype)
            v = live_view(case, out)
            v.copy_(v + y if case.accumulate else y)
        outs.append(out)
    return outs
