"""The ownership rule of the host files ("Ownership"), without a device.

test_owners_against_a_fake_runtime builds tests/host/hip_owner_check.cpp -- xfr_amd/csrc/hip_owner.h against the stand-in hip/hip_runtime.h beside it
-- with the host compiler under AddressSanitizer and UBSan, and runs it: ownership, grow, failed creations, all-or-nothing groups, status mapping,
and the guard of xfr_amd/csrc/scoped.h (a scope's value goes back on every way out).
test_raw_lifetime_calls_live_in_the_owner_header reads the sources: outside hip_owner.h nothing creates or destroys a device resource by hand.
test_call_state_is_not_engine_state reads them for DESIGN.md section 9m: a sweep's context and the one-shots of a call are arguments, not members of
the engine; no .hip file defines a guard of its own; nobody can call the sweep without saying which context it runs in."""
import glob
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'xfr_amd', 'csrc')
HOST = os.path.join(ROOT, 'tests', 'host')
RAW = re.compile(r'\b(hipFree|hipHostFree|hipEventDestroy|hipStreamDestroy|hipMalloc|hipHostMalloc|hipEventCreate\w*|hipStreamCreate\w*)\s*\(')
# the two places that keep a raw call: the process-lifetime tail workspace of xfr_debug_conv (one line), and the plane cache of the bf16x6 kernel file
TWS_LINE = re.compile(r'hipMalloc\(&tws,')
KERNEL_CACHE = 'conv_gemm_split.hip'


def test_owners_against_a_fake_runtime(tmp_path):
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    assert cxx, 'no host C++ compiler found'
    exe = str(tmp_path / 'hip_owner_check')
    # the sanitizers' runtimes inside the program (clang's default; asked of gcc): it runs the same whatever else the environment loads into a process
    version = subprocess.run([cxx, '--version'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True).stdout
    static = [] if 'clang' in version else ['-static-libasan', '-static-libubsan']
    build = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined'] + static + ['-I', HOST, os.path.join(HOST, 'hip_owner_check.cpp'),
                            '-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout


def test_raw_lifetime_calls_live_in_the_owner_header():
    found = []
    files = sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h')))
    assert os.path.join(CSRC, 'hip_owner.h') in files and len(files) > 20
    tws = 0
    for path in files:
        base = os.path.basename(path)
        if base in ('hip_owner.h', KERNEL_CACHE):
            continue
        for no, line in enumerate(open(path), 1):
            if not RAW.search(line):
                continue
            if base == 'debug_abi.hip' and TWS_LINE.search(line) and len(RAW.findall(line)) == 1:
                tws += 1
                continue
            found.append('%s:%d: %s' % (base, no, line.strip()))
    assert not found, 'raw lifetime calls outside hip_owner.h:\n' + '\n'.join(found)
    assert tws == 1, 'the tail workspace of xfr_debug_conv is one line'
    owner = open(os.path.join(CSRC, 'hip_owner.h')).read()
    assert len(set(m.group(1) for m in RAW.finditer(owner))) == 9      # every one of them lives there (both stream creations)


# what one call used to leave on the engine for its callees to read back
PER_CALL = ('rc_priors', 'rc_caps', 'rc_prior_row', 'rc_cap_row', 'rc_dense_slot', 'rc_prior_dense', 'rc_active', 'rc_n', 'lazy_zero', 'store_slot', 'tab_sb',
            'store_tensor', 'store_sb', 'inputs_event', 'stage_slot')


def _strip_comments(text):
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def _braced(text, start):
    """The text between the brace that follows `start` and its partner."""
    i = text.index('{', start)
    depth = 0
    for j in range(i, len(text)):
        depth += {'{': 1, '}': -1}.get(text[j], 0)
        if depth == 0:
            return text[i + 1:j]
    raise AssertionError('unbalanced braces')


def test_call_state_is_not_engine_state():
    header = _strip_comments(open(os.path.join(CSRC, 'engine_internal.h')).read())
    body = _braced(header, header.index('struct xfr_engine'))
    assert 'cur_slot' in body and 'hold_forward' in body and len(body) > 4000          # (the engine's body it is)
    declared = set(re.findall(r'[A-Za-z_]\w*', body))
    assert not declared & set(PER_CALL), 'per-call state declared on the engine: %s' % sorted(declared & set(PER_CALL))
    # one guard type (scoped.h) and HoldGuard beside it in the header: none defined inside a function of a .hip file
    local = []
    for path in sorted(glob.glob(os.path.join(CSRC, '*.hip'))):
        for m in re.finditer(r'\bstruct\s+(\w*Guard|Unpipe)\b\s*[{:]', _strip_comments(open(path).read())):
            local.append('%s: struct %s' % (os.path.basename(path), m.group(1)))
    assert not local, 'guard structs defined in .hip files:\n' + '\n'.join(local)
    assert re.search(r'\bclass\s+Scoped\b', open(os.path.join(CSRC, 'scoped.h')).read()) and '#include "scoped.h"' in header
    assert 'hip/' not in open(os.path.join(CSRC, 'scoped.h')).read()                 # the host compiler alone builds it
    # the sweep's context is an explicit argument: a SweepCtx parameter without a default in each declaration
    for fn in ('run_backward', 'resolve_chain', 'bwd_conv_params', 'lean_applies', 'ebp_core'):
        m = re.search(r'\b%s\s*\(([^;{]*)\)\s*;' % fn, header)
        assert m, 'no declaration of %s in engine_internal.h' % fn
        params = [p.strip() for p in m.group(1).split(',')]
        ctx = [p for p in params if 'SweepCtx' in p]
        assert len(ctx) == 1 and '=' not in ctx[0], '%s(%s)' % (fn, m.group(1))
