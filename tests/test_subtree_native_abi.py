"""The C-ABI side of weighted subtree EBP in one call (xfr_weighted_subtree_ebp): declared, bound and exported; the xfr_subtree_args
mirror of the ctypes binding has the header's layout; examples/c_subtree.c compiles as C99 against the header alone, links against
libxfr_amd.so, and without a HIP device fails loudly instead of falling back."""
import ctypes
import os
import re
import subprocess

import torch

from xfr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'xfr_amd', 'csrc')


def _gcc(src, exe, extra=()):
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), src] + list(extra) + ['-o', exe])
    return exe


def test_entry_point_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'xfr_amd.h')).read()
    assert re.search(r'xfr_status\s+xfr_weighted_subtree_ebp\s*\(', hdr)
    assert '#define XFR_AMD_ABI_VERSION 7' in hdr and _lib.ABI_VERSION == 7
    assert 'xfr_weighted_subtree_ebp' in [n for n, _, _ in _lib.SYMBOLS]
    lib = _lib.load()
    assert hasattr(lib, 'xfr_weighted_subtree_ebp') and lib.xfr_abi_version() == 7


def test_subtree_args_layout_matches_header(tmp_path):
    src = tmp_path / 'layout.c'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "xfr_amd.h"\n'
                   'int main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(xfr_subtree_args), offsetof(xfr_subtree_args, topk),\n'
                   '           offsetof(xfr_subtree_args, gate_ge0), offsetof(xfr_subtree_args, do_max_subtree), offsetof(xfr_subtree_args, output),\n'
                   '           offsetof(xfr_subtree_args, sweep_batch), offsetof(xfr_subtree_args, order_fn), offsetof(xfr_subtree_args, order_user));\n'
                   '    printf("%d %d %d\\n", (int)XFR_SUBTREE_MWP, (int)XFR_SUBTREE_SALIENCY, (int)XFR_SUBTREE_UINT8);\n'
                   '    return 0;\n}\n')
    exe = _gcc(str(src), str(tmp_path / 'layout'))
    lines = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split('\n')
    want = [int(v) for v in lines[0].split()]
    A = _lib.SubtreeArgs
    got = [ctypes.sizeof(A)] + [getattr(A, f).offset for f in ('topk', 'gate_ge0', 'do_max_subtree', 'output', 'sweep_batch', 'order_fn', 'order_user')]
    assert got == want, (got, want)
    assert [int(v) for v in lines[1].split()] == [_lib.SUBTREE_MWP, _lib.SUBTREE_SALIENCY, _lib.SUBTREE_UINT8]


def test_c_subtree_example_compiles_links_and_fails_loudly_without_a_device(tmp_path):
    exe = _gcc(os.path.join(ROOT, 'examples', 'c_subtree.c'), str(tmp_path / 'c_subtree'),
               ['-L' + CSRC, '-lxfr_amd', '-Wl,-rpath,' + CSRC, '-ldl', '-lm'])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    if not torch.cuda.is_available():
        assert 'no CPU fallback' in out.stdout
    else:
        assert "firings among the reference's yes" in out.stdout


def test_arguments_are_checked_before_any_device_work():
    lib = _lib.load()
    args = _lib.SubtreeArgs(8, 1, 0, _lib.SUBTREE_MWP, 0, _lib.SUBTREE_ORDER_FN(), None)
    st = lib.xfr_weighted_subtree_ebp(None, None, 1, 5, None, ctypes.byref(args), None, None, None, None, None, None)
    assert st == _lib.XFR_INVALID_ARG and b'null engine' in lib.xfr_last_error()
