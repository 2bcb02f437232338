"""The C-ABI side of the uint8 saliency tail: xfr_mwp_to_saliency_u8, xfr_contrastive_u8, xfr_triplet_contrastive_u8tail and
XFR_SUBTREE_UINT8_SALIENCY are declared in the header, exported by the library and bound with the header's argument types; the ABI version stays 7;
the existing values of xfr_subtree_output keep their numbers.  No device needed."""
import ctypes
import os
import re
import subprocess

from xfr_amd import _lib
from xfr_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
# name -> (the header's parameter types in order, the binding's argtypes)
NEW = {
    'xfr_mwp_to_saliency_u8': (['xfr_engine*', 'const float*', 'const uint8_t*', 'int32_t', 'int32_t', 'int32_t', 'uint8_t*', 'void*'],
                               [P, P, P, I, I, I, P, P]),
    'xfr_contrastive_u8': (['xfr_engine*', 'const float*', 'int32_t', 'int32_t', 'const float*', 'float', 'uint8_t*', 'void*'],
                           [P, P, I, I, P, F, P, P]),
    'xfr_triplet_contrastive_u8tail': (['xfr_engine*', 'const float*', 'const float*', 'int32_t', 'int32_t', 'float', 'float', 'uint8_t*', 'void*',
                                        'int32_t'], [P, P, P, I, I, F, F, P, P, I]),
}


def _header():
    return open(os.path.join(ROOT, 'include', 'xfr_amd.h')).read()


def _declared_types(hdr, name):
    m = re.search(r'xfr_status\s+%s\s*\(([^;]*?)\)\s*;' % name, hdr)
    assert m, '%s is not declared' % name
    return [re.sub(r'\s*\w+$', '', re.sub(r'\s+', ' ', a).strip()).replace(' *', '*') for a in m.group(1).split(',')]


def test_new_symbols_are_declared_exported_and_bound():
    hdr = _header()
    assert '#define XFR_AMD_ABI_VERSION 7' in hdr and _lib.ABI_VERSION == 7
    lib = _lib.load()
    assert lib.xfr_abi_version() == 7
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name, (types, argtypes) in NEW.items():
        assert _declared_types(hdr, name) == types, (name, _declared_types(hdr, name))
        assert name in bound and bound[name][0] is I and list(bound[name][1]) == argtypes, name
        fn = getattr(lib, name)
        assert fn.restype is I and list(fn.argtypes) == argtypes


def test_existing_variants_are_untouched():
    """The uint8-INPUT variants keep their names and signatures beside the new uint8-OUTPUT one."""
    hdr = _header()
    for name in ('xfr_triplet_contrastive_u8', 'xfr_triplet_contrastive_u8_host', 'xfr_contrastive_raw', 'xfr_mwp_to_saliency'):
        assert re.search(r'xfr_status\s+%s\s*\(' % name, hdr) and name in [n for n, _, _ in _lib.SYMBOLS]
    assert _declared_types(hdr, 'xfr_triplet_contrastive_u8')[1] == 'const uint8_t*'
    assert 'stays with the caller' not in hdr and 'on the host. */' not in hdr[hdr.index('xfr_contrastive_raw') - 600:hdr.index('xfr_contrastive_raw')]


def test_subtree_output_enum(tmp_path):
    src = tmp_path / 'enum.c'
    src.write_text('#include <stdio.h>\n#include "xfr_amd.h"\nint main(void) {\n'
                   '    printf("%d %d %d %d\\n", (int)XFR_SUBTREE_MWP, (int)XFR_SUBTREE_SALIENCY, (int)XFR_SUBTREE_UINT8, (int)XFR_SUBTREE_UINT8_SALIENCY);\n'
                   '    return 0;\n}\n')
    exe = str(tmp_path / 'enum')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [0, 1, 2, 3] == [_lib.SUBTREE_MWP, _lib.SUBTREE_SALIENCY, _lib.SUBTREE_UINT8, _lib.SUBTREE_UINT8_SALIENCY]
    assert Engine.SUBTREE_OUTPUTS['uint8_saliency'] == 3 and Engine.SUBTREE_OUTPUTS['uint8'] == 2


def test_arguments_are_checked_before_any_device_work():
    lib = _lib.load()
    assert lib.xfr_mwp_to_saliency_u8(None, None, None, 1, 4, 4, None, None) == _lib.XFR_INVALID_ARG
    assert b'xfr_mwp_to_saliency_u8' in lib.xfr_last_error()
    assert lib.xfr_contrastive_u8(None, None, 1, 2, None, -1.0, None, None) == _lib.XFR_INVALID_ARG
    assert lib.xfr_triplet_contrastive_u8tail(None, None, None, 1, 2, 1.0, -1.0, None, None, 0) == _lib.XFR_INVALID_ARG


def test_python_surface_has_the_keywords():
    import inspect
    from xfr_amd import inpainting_game as IG
    from xfr_amd.models.whitebox import Whitebox
    assert inspect.signature(Engine.contrastive).parameters['tail'].default == 'v6'
    assert inspect.signature(Engine.triplet_contrastive).parameters['tail'].default == 'v6'
    assert hasattr(Engine, 'mwp_to_saliency_u8')
    for fn in (Whitebox.contrastive_triplet_ebp_batch, Whitebox.triplet_images_ebp_batch, Whitebox.weighted_subtree_ebp_batch, IG.run_jobs_batched):
        assert inspect.signature(fn).parameters['tail'].default == 'v6', fn
    assert 'ebp_version 6 maps (float32) for the batched tails' not in IG.run_jobs_batched.__doc__
