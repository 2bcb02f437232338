"""The ownership rule of the host files ("Ownership"), without a device.

test_owners_against_a_fake_runtime builds tests/host/hip_owner_check.cpp -- xfr_amd/csrc/hip_owner.h against the stand-in hip/hip_runtime.h beside it
-- with the host compiler under AddressSanitizer and UBSan, and runs it: ownership, grow, failed creations, all-or-nothing groups, status mapping.
test_raw_lifetime_calls_live_in_the_owner_header reads the sources: outside hip_owner.h nothing creates or destroys a device resource by hand."""
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
