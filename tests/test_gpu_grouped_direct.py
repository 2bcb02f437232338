"""Single launches of the depthwise kernel (xfr_amd/csrc/conv_depthwise.hip, configuration 14) and the grouped MFMA kernel (conv_group.hip,
configuration 13) through xfr_debug_conv_grouped, on the cases of tests/grouped_direct_cases.py: the branches no layer catalogue reaches -- the RB = 4
template and its dead row blocks, the VEC output path across tiles, the tile fallbacks 512 / 256 / 128 and "no tile", CO 2 and CO 8, Ci 8, the caps, the
alignment fallbacks, pad_dw of both signs, the scattered store from both decodes, accumulate on the 16-byte path.

Every launch is held to the float64 reference (grouped_direct_cases.reference) under the rule of tests/parity_harness.py, e_eng <= max(4 e32, 2e-6), on
the elements it writes; every depthwise-eligible case on BOTH kernels (cfg 0, which must pick 14 with the tile the table states, and cfg 13), each
against float64, not against the other.  Around that: the configuration and tile the library reports; nothing else written (a margin in front of and
behind every output, the images nb .. out_nb - 1, the holes of a scattered target and out1 of a one-half launch keep the bits of their pattern; a
refused cfg-14 call leaves everything); nothing else read into a live output (the input's margins and its images nb .. in_nb - 1 are NaN, every
output is finite); two launches give the same bits; and one inf in one group's input leaves every other group's outputs bit-identical.
XFR_LAYER_PARITY_REPORT=<path> adds every measured (e_eng, e32) pair to that file under direct/<case>/cfg<13|14>/out<0|1>.

Measured on the MI355X over the 119 comparisons of this file: e32 at most 5.26e-7 (tm512), e_eng at most 6.50e-7 (rb4_back/nb2 on configuration 13,
out0, against e32 1.48e-7: under the 2e-6 floor at 33 % of it, the tightest comparison of the file, and the largest e_eng / e32, 4.4); on configuration
14 e_eng at most 5.26e-7 (tm512, equal to its e32: 25 % of its bound 4 x e32).  On every depthwise-eligible case configurations 13 and 14 give the same
e_eng to the printed digits.  Inputs and seeds are fixed and the kernels deterministic, so the margins repeat run to run.  Four value-only mutants of the
kernels (the stride dropped from the VEC decode; the bias on three of four lanes of the 16-byte store; oh_lo = 0 for a tile's first image; row block 3
not stored) each fail this file: DESIGN.md section 9l lists the cases.
"""
import ctypes

import pytest
import torch

import grouped_direct_cases as C
import parity_harness as H
from xfr_amd import _lib

pytestmark = pytest.mark.gpu

h = H.Harness(print_check=True)
_inputs = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    h.finish('XFR_LAYER_PARITY_REPORT', merge=True)


def _inp(case):
    """The case's inputs and references, computed once: inputs(), r32 / r64 = (out0, out1) of the float32 oracle and the float64 reference."""
    if case.name not in _inputs:
        inp = C.inputs(case)
        inp['r64'] = C.reference(case, inp, torch.float64)
        inp['r32'] = C.reference(case, inp, torch.float32)
        _inputs[case.name] = inp
    return _inputs[case.name]


def _flat(t, shift, margin):
    """t in a flat buffer with MARGIN + shift floats in front and MARGIN behind, all holding `margin` (a tensor of that many values, or a number)."""
    n = t.numel()
    buf = torch.empty(C.MARGIN + shift + n + C.MARGIN, dtype=torch.float32)
    head = C.MARGIN + shift
    if torch.is_tensor(margin):
        buf[:head] = margin[:head]
        buf[head + n:] = margin[head:head + C.MARGIN]
    else:
        buf[:head] = margin
        buf[head + n:] = margin
    buf[head:head + n] = t.reshape(-1)
    return buf


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch(case, inp, cfg, device, x=None):
    """One xfr_debug_conv_grouped call on fresh buffers -> (status, cfg_out, tile_out, [flat out0, flat out1] on the CPU, [their states before])."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(case.seed + 2)
    xin = _flat(inp['x'] if x is None else x, case.in_shift, float('nan')).to(device)
    before = [_flat(inp['pre%d' % k], case.out_shift, torch.rand(2 * C.MARGIN + 8, generator=g) * 2 - 1) for k in range(2)]
    outs = [b.to(device) for b in before]
    assert xin.data_ptr() % 16 == 0 and outs[0].data_ptr() % 16 == 0 and outs[1].data_ptr() % 16 == 0
    origin = case.origin[0] * case.target[1] + case.origin[1]
    ptr = lambda buf, shift, extra=0: buf.data_ptr() + 4 * (C.MARGIN + shift + extra)
    bias = None if inp['bias'] is None else inp['bias'].contiguous().data_ptr()
    bias_pos = None if inp['bias_pos'] is None else inp['bias_pos'].contiguous().data_ptr()
    cfg_out, tile_out = ctypes.c_int32(-1), ctypes.c_int32(-1)
    torch.cuda.synchronize()
    st = lib.xfr_debug_conv_grouped(ptr(xin, case.in_shift), ptr(outs[0], case.out_shift, origin), ptr(outs[1], case.out_shift, origin), inp['w'].data_ptr(),
                                    bias, bias_pos, case.cin, case.cout, case.G, case.H, case.W, case.NB, case.in_nb, case.out_nb, case.kh, case.kw,
                                    case.stride, case.pad, case.pad_dw, case.relu_in, case.nhalves, case.accumulate, case.out_stride,
                                    0 if case.dense else case.target[0], 0 if case.dense else case.target[1], cfg, ctypes.byref(cfg_out), ctypes.byref(tile_out))
    torch.cuda.synchronize()
    return st, cfg_out.value, tile_out.value, [o.cpu() for o in outs], before


def _tensor(case, flat):
    head = C.MARGIN + case.out_shift
    n = case.cout * case.out_nb * case.target[0] * case.target[1]
    return flat[head:head + n].view(case.cout, case.out_nb, case.target[0], case.target[1])


def _check_launch(bad, case, inp, cfg, want_cfg, want_tile, device):
    """One launch under every check of this file but isolation; messages go to `bad`."""
    tag = '%s/cfg%d' % (case.name, want_cfg)
    st, ran, tile, outs, before = _launch(case, inp, cfg, device)
    if st != _lib.XFR_OK:
        bad.append('%s: status %d: %s' % (tag, st, _lib.load().xfr_last_error().decode()))
        return
    if (ran, tile) != (want_cfg, want_tile):
        bad.append('%s: configuration %d with tile %d ran, the table states %d with tile %d' % (tag, ran, tile, want_cfg, want_tile))
    head = C.MARGIN + case.out_shift
    live = torch.zeros((case.cout, case.out_nb) + tuple(case.target), dtype=torch.bool)
    C.live_view(case, live).fill_(True)
    for k in range(2):
        got = _tensor(case, outs[k])
        n = got.numel()
        if not (torch.equal(_bits(outs[k][:head]), _bits(before[k][:head])) and torch.equal(_bits(outs[k][head + n:]), _bits(before[k][head + n:]))):
            bad.append('%s: out%d: the margin around the tensor was written' % (tag, k))
        if k >= case.nhalves:
            if not torch.equal(_bits(got), _bits(inp['pre%d' % k])):
                bad.append('%s: out1 of a one-half launch was written' % tag)
            continue
        if not torch.equal(_bits(got[~live]), _bits(inp['pre%d' % k][~live])):
            bad.append('%s: out%d: elements outside the launch (images beyond nb, holes of the target) were written' % (tag, k))
        h.check(bad, 'direct/%s/out%d' % (tag, k), C.live_view(case, got), C.live_view(case, inp['r32'][k]), C.live_view(case, inp['r64'][k]))
    again = _launch(case, inp, cfg, device)
    if again[0] != _lib.XFR_OK or not all(torch.equal(_bits(a), _bits(b)) for a, b in zip(outs, again[3])):
        bad.append('%s: a second launch gave other bits' % tag)


@pytest.mark.parametrize('name', [c.name for c in C.CASES])
def test_launch_matches_float64(gpu_device, name):
    """The case on the configuration cfg 0 picks (which, and with which tile, as the table states), and every depthwise-eligible case on configuration 13
    as well; a case the depthwise kernel refuses is refused at cfg 14 with XFR_UNSUPPORTED_LAYER and every byte of both buffers as it was."""
    case = C.BY_NAME[name]
    inp = _inp(case)
    bad = []
    want_cfg, want_tile = case.expect
    grouped = case in C.GROUPED
    _check_launch(bad, case, inp, C.CFG_GROUP if grouped else 0, want_cfg, want_tile, gpu_device)
    if case.eligible:
        _check_launch(bad, case, inp, C.CFG_DEPTHWISE, C.CFG_DEPTHWISE, want_tile, gpu_device)
        _check_launch(bad, case, inp, C.CFG_GROUP, C.CFG_GROUP, 0, gpu_device)
    elif not grouped:
        st, ran, tile, outs, before = _launch(case, inp, C.CFG_DEPTHWISE, gpu_device)
        if st != _lib.XFR_UNSUPPORTED_LAYER or (ran, tile) != (0, 0):
            bad.append('%s: cfg 14 gave status %d, configuration %d, tile %d: a refusal was due' % (name, st, ran, tile))
        if not all(torch.equal(_bits(a), _bits(b)) for a, b in zip(outs, before)):
            bad.append('%s: the refused cfg-14 call wrote to an output buffer' % name)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name', C.ISOLATION)
def test_groups_stay_apart(gpu_device, name):
    """One +inf in one input element of group 1: the group's own outputs are not all finite, every other group's have the bits of the finite run."""
    case = C.BY_NAME[name]
    inp = _inp(case)
    cfg = C.CFG_GROUP if case in C.GROUPED else 0
    hot = inp['x'].clone()
    hot[case.Ci + case.Ci // 2, 0, case.H // 2, case.W // 2] = float('inf')
    a, b = _launch(case, inp, cfg, gpu_device), _launch(case, inp, cfg, gpu_device, x=hot)
    assert a[0] == b[0] == _lib.XFR_OK and a[1] == b[1] == case.expect[0]
    own = slice(case.Co, 2 * case.Co)
    others = [c for c in range(case.cout) if not case.Co <= c < 2 * case.Co]
    for k in range(case.nhalves):
        fin, poi = _tensor(case, a[3][k]), _tensor(case, b[3][k])
        assert bool(torch.isfinite(fin).all())
        assert not bool(torch.isfinite(poi[own]).all())                      # the poison did arrive
        assert torch.equal(_bits(fin[others]), _bits(poi[others]))
        assert torch.equal(_bits(fin[own, 1:]), _bits(poi[own, 1:]))         # ... and stayed in its image
