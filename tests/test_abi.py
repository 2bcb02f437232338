"""The C-ABI boundary: the shared library loads and exports exactly what include/xfr_amd.h declares, the ctypes
mirror of the structs matches, and the product path fails loudly without a HIP device (no CPU fallback)."""
import ctypes
import os
import re

import pytest
import torch

from xfr_amd import _lib
from xfr_amd.program import OpDesc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, 'include', 'xfr_amd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(xfr_[a-z_0-9]+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    declared = header_functions()
    bound = sorted(n for n, _, _ in _lib.SYMBOLS)
    assert declared == bound, 'header and ctypes binding disagree: %s' % (set(declared) ^ set(bound))
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.xfr_abi_version() == _lib.ABI_VERSION


def test_elementwise_launch_stats_need_no_device():
    """xfr_elementwise_launch_stats / xfr_elementwise_variant_name: a name per counter, NULL beyond the last, short and missing buffers."""
    lib = _lib.load()
    n = ctypes.c_int32(-1)
    assert lib.xfr_elementwise_launch_stats(None, 0, ctypes.byref(n)) == _lib.XFR_OK and n.value > 0
    names = _lib.elementwise_variant_names()
    assert len(names) == n.value == len(set(names))
    assert lib.xfr_elementwise_variant_name(n.value) is None and lib.xfr_elementwise_variant_name(-1) is None
    two = (ctypes.c_int64 * 3)(-7, -7, -7)
    assert lib.xfr_elementwise_launch_stats(two, 2, None) == _lib.XFR_OK
    assert two[0] >= 0 and two[1] >= 0 and two[2] == -7
    assert lib.xfr_elementwise_launch_stats(None, 2, None) == _lib.XFR_INVALID_ARG
    assert lib.xfr_elementwise_launch_stats(two, -1, None) == _lib.XFR_INVALID_ARG
    stats = _lib.elementwise_launch_stats()
    assert sorted(stats) == sorted(names) and all(v >= 0 for v in stats.values())


def test_opdesc_layout():
    assert ctypes.sizeof(OpDesc) == 16 * 4
    assert OpDesc.fparam.offset == 11 * 4 and OpDesc.w_var.offset == 15 * 4


def test_error_strings_and_arg_checks():
    lib = _lib.load()
    h = ctypes.c_void_p()
    st = lib.xfr_engine_create(None, 0, 0, 3, 224, 224, 1, 0, ctypes.byref(h))
    assert st == _lib.XFR_INVALID_ARG
    assert b'bad arguments' in lib.xfr_last_error()
    assert lib.xfr_engine_set_mode(None, 1, 1e-16, 0) == _lib.XFR_INVALID_ARG


def test_debug_contrast_tail_refuses_before_any_device_call():
    """xfr_debug_contrast_tail checks its arguments before it touches the engine or the device, so the refusals show without either: the pointers
    here are numbers that are never followed.  (tests/test_gpu_contrast_tail.py repeats them on real buffers and proves nothing was written.)"""
    lib = _lib.load()
    e, p, s, t, o = 1 << 20, 1 << 24, 1 << 28, 1 << 29, 1 << 30

    def refused(text, e=e, p=p, c=3, n=2, hw=8, pct=20.0, s=s, t=t, o=o):
        assert lib.xfr_debug_contrast_tail(e, p, c, n, hw, pct, s, t, o, None) == _lib.XFR_INVALID_ARG
        assert text in lib.xfr_last_error(), lib.xfr_last_error()

    refused(b'null argument', e=None)
    refused(b'null argument', p=None)
    refused(b'null argument', o=None)
    refused(b'c 0, n 2, hw 8', c=0)
    refused(b'c 3, n -2, hw 8', n=-2)
    refused(b'c 3, n 2, hw 0', hw=0)
    refused(b'percentile 100.5', pct=100.5)
    refused(b'nan', pct=float('nan'))
    refused(b'p_dev 0x1000004 is not 16-byte aligned', p=p + 4)
    refused(b'sums_dev 0x1000010 (32 bytes) overlaps p_dev 0x1000000', s=p + 16)
    refused(b'thr_dev 0x100017c (8 bytes) overlaps p_dev', t=p + 4 * 3 * 4 * 8 - 4)
    refused(b'contrast_dev 0xffffc4 (64 bytes) overlaps p_dev', o=p - 60)


def test_debug_conv_grouped_refuses_before_any_device_call():
    """xfr_debug_conv_grouped checks its arguments before it allocates, copies or launches, so the refusals show without a device: the device pointers
    are numbers that are never followed, the weight is real host memory that is never read.  (tests/test_gpu_grouped_direct.py runs the launches.)"""
    lib = _lib.load()
    w = (ctypes.c_float * (8 * 2 * 9))()
    x, o0, o1 = 1 << 24, 1 << 28, 1 << 29
    good = dict(x=x, o0=o0, o1=o1, w=ctypes.addressof(w), cin=8, cout=8, groups=4, h=9, wd=8, nb=2, in_nb=2, out_nb=2, kh=3, kw=3, stride=1, pad=1, pad_dw=0,
                relu_in=0, nhalves=2, accumulate=0, out_stride=1, out_H=0, out_W=0, cfg=0)

    def refused(text, **kw):
        a = dict(good, **kw)
        cfg_out, tile_out = ctypes.c_int32(-1), ctypes.c_int32(-1)
        st = lib.xfr_debug_conv_grouped(a['x'], a['o0'], a['o1'], a['w'], None, None, a['cin'], a['cout'], a['groups'], a['h'], a['wd'], a['nb'], a['in_nb'],
                                        a['out_nb'], a['kh'], a['kw'], a['stride'], a['pad'], a['pad_dw'], a['relu_in'], a['nhalves'], a['accumulate'],
                                        a['out_stride'], a['out_H'], a['out_W'], a['cfg'], ctypes.byref(cfg_out), ctypes.byref(tile_out))
        assert st == _lib.XFR_INVALID_ARG, (text, st)
        assert text in lib.xfr_last_error(), lib.xfr_last_error()
        assert (cfg_out.value, tile_out.value) == (0, 0)

    refused(b'null argument', x=None)
    refused(b'null argument', o0=None)
    refused(b'null argument', w=None)
    refused(b'nhalves 2, out1_dev (nil)', o1=None)
    refused(b'nhalves 3', nhalves=3)
    refused(b'nhalves 0', nhalves=0)
    refused(b'cfg 12', cfg=12)
    refused(b'cfg 9', cfg=9)
    refused(b'cin 8, cout 8, groups 1', groups=1)
    refused(b'cin 8, cout 8, groups 3', groups=3)
    refused(b'cin 8, cout 6, groups 4', cout=6)
    refused(b'h 0, w 8', h=0)
    refused(b'kh 3, kw 0', kw=0)
    refused(b'stride 0', stride=0)
    refused(b'nb 0, in_nb 2, out_nb 2', nb=0)
    refused(b'nb 3, in_nb 2, out_nb 4', nb=3, out_nb=4)
    refused(b'nb 3, in_nb 4, out_nb 2', nb=3, in_nb=4)
    refused(b'relu_in 2, accumulate 0', relu_in=2)
    refused(b'relu_in 0, accumulate -1', accumulate=-1)
    refused(b'pad -4, pad_dw 0 leave no output', pad=-4)
    refused(b'pad 1, pad_dw -4 leave no output', pad_dw=-4)
    refused(b'out_stride 2, out_H 0, out_W 0', out_stride=2)
    refused(b'out_stride 1, out_H 9, out_W 0', out_H=9)
    refused(b'out_stride 2, out_H 17, out_W 14 do not hold the 9 x 8 outputs', out_stride=2, out_H=17, out_W=14)
    refused(b'out_stride 2, out_H 16, out_W 15 do not hold the 9 x 8 outputs', out_stride=2, out_H=16, out_W=15)
    refused(b'out_stride 0', out_stride=0)
    refused(b'2^31 elements', in_nb=1 << 30, nb=2)


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_no_gpu_means_loud_failure_not_fallback():
    from parity_utils import make_backbone, make_images
    from xfr_amd.models import whitebox as WB
    bb, _ = make_backbone('stresnet_mini')
    wb = WB.Whitebox(WB.WhiteboxSTResnet(bb))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        wb.net.encode(make_images('stresnet_mini', 1))
    prog = bb.build_program()
    h = ctypes.c_void_p()
    st = _lib.load().xfr_engine_create(prog.op_array(), len(prog.ops), len(prog.weight_names), 3, 224, 224, 1, 0, ctypes.byref(h))
    assert st == _lib.XFR_HIP_ERROR and b'no CPU fallback' in _lib.load().xfr_last_error()


def test_whitebox_constructor_errors_match_reference():
    from parity_utils import make_backbone
    from xfr_amd.models import whitebox as WB
    bb, _ = make_backbone('stresnet_mini')
    net = WB.WhiteboxSTResnet(bb)
    with pytest.raises(RuntimeError, match='at least 4'):        # whitebox.py:283-284
        WB.Whitebox(net, ebp_version=3)
    with pytest.raises(ValueError, match='Invalid subtree mode'):  # whitebox.py:430
        WB.Whitebox(net, ebp_subtree_mode='bogus')
    with pytest.raises(AssertionError):                           # whitebox.py:275
        WB.Whitebox(bb)
    wb = WB.Whitebox(net, ebp_version=11)
    assert wb._ebp_with_bias is True and wb.convert_saliency_uint8 is True      # whitebox.py:285-289
    assert WB.Whitebox(net).ebp_subtree_mode() == 'affineonly_with_prior' and WB.Whitebox(net).eps == 1e-16


def _build_c_host(tmp_path):
    import subprocess
    exe = str(tmp_path / 'c_host')
    csrc = os.path.join(ROOT, 'xfr_amd', 'csrc')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'examples', 'c_host.c'),
                           '-L' + csrc, '-lxfr_amd', '-Wl,-rpath,' + csrc, '-ldl', '-lm', '-o', exe])
    return exe


def test_header_is_plain_c_and_a_c_host_links(tmp_path):
    """include/xfr_amd.h is C99 (no C++ or torch types at the boundary): examples/c_host.c compiles with gcc -std=c99 against
    it, links against libxfr_amd.so alone and runs -- the planner everywhere, the engine where a HIP device is visible."""
    import subprocess
    exe = _build_c_host(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'fused schedule' in out.stdout and 'bwd CONV_BWD' in out.stdout
    if not torch.cuda.is_available():
        assert 'no CPU fallback' in out.stdout


@pytest.mark.gpu
def test_c_host_runs_contrastive_ebp(tmp_path):
    import re
    import subprocess
    out = subprocess.run([_build_c_host(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r'saliency map 16x16: sum ([0-9.]+), max ([0-9.]+)', out.stdout)
    assert m and abs(float(m.group(1)) - 1.0) < 1e-4 and float(m.group(2)) > 0
    # ... and the program itself compared its encodings and its map with what the REAL reference computes for the same network, parameters and
    # images (examples/c_host_ref.h, generated by tests/golden/make_golden_chost.py); exit code 0 means 1e-3 / cosine 0.99999 held
    r = re.search(r'against the reference: encodings max\|d\| ([0-9.e+-]+), map max\|d\|/max ([0-9.e+-]+), cosine ([0-9.]+)', out.stdout)
    assert r and float(r.group(1)) < 1e-5 and float(r.group(2)) <= 1e-3 and float(r.group(3)) >= 0.99999, out.stdout
