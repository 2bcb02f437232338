#!/usr/bin/env python
"""Digest of the device code of the kernel files, for checking a kernel refactor to the instruction.  Needs hipcc, no GPU:

    python tools/isa_digest.py > before.txt       # on the old tree
    python tools/isa_digest.py > after.txt        # on the new one; `diff before.txt after.txt` must be empty

Every file is compiled with the Makefile's flags plus `--cuda-device-only -S`.  One line per kernel: the sha256 of its instruction stream (label to
.Lfunc_end, comments and blank lines stripped, the function index taken out of local labels and the kernel's own name out of its descriptor, so
that a kernel that only changed its name, as a template instantiation does, keeps its hash), its name and its resource figures; a total over all of
them follows.  --dump DIR also writes each kernel's normalised text, to see what moved.
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'xfr_amd', 'csrc')
DEFAULT_FILES = ('conv_gemm.hip', 'conv_gemm_split.hip', 'elementwise.hip', 'strise.hip', 'inpaint.hip', 'saliency.hip', 'match.hip', 'finish.hip', 'intake.hip', 'u8_tail.hip', 'conv_depthwise.hip')
FIGURES = (('vgpr', 'NumVgprs'), ('agpr', 'NumAgprs'), ('sgpr', '(?:Total)?NumSgprs'), ('scratch', 'ScratchSize'), ('lds', 'LDSByteSize'), ('occupancy', 'Occupancy'))


def makefile_flags():
    """CXXFLAGS of xfr_amd/csrc/Makefile with its own $(ARCH): the digest is of what `make` builds."""
    text = open(os.path.join(CSRC, 'Makefile')).read()
    var = lambda name: re.search(r'^%s\s*\??=\s*(.*)$' % name, text, re.M).group(1).strip()
    return var('CXXFLAGS').replace('$(ARCH)', os.environ.get('ARCH', var('ARCH'))).split()


def compile_asm(path, jobs_dir):
    out = os.path.join(jobs_dir, os.path.basename(path) + '.s')
    cmd = [os.environ.get('HIPCC', 'hipcc')] + makefile_flags() + ['--cuda-device-only', '-S', path, '-o', out]
    done = subprocess.run(cmd, cwd=os.path.dirname(path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if done.returncode != 0:
        sys.exit('isa_digest: %s failed:\n%s' % (' '.join(cmd), done.stdout))
    return open(out).read()


def kernels_of(asm):
    """{kernel name: (normalised instruction text, {figure: value})} of one assembly file."""
    lines = asm.splitlines()
    names = set(m.group(1) for m in (re.match(r'\s*\.amdhsa_kernel\s+(\S+)', l) for l in lines) if m)
    found = {}
    i = 0
    while i < len(lines):
        m = re.match(r'([A-Za-z_$][\w$.]*):', lines[i])
        if not (m and m.group(1) in names):
            i += 1
            continue
        name, body = m.group(1), []
        i += 1
        while i < len(lines) and not re.match(r'\.Lfunc_end\d+:', lines[i]):
            code = lines[i].split(';', 1)[0].strip()
            if code:
                body.append(re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r'\s+', ' ', code)).replace(name, '<kernel>'))
            i += 1
        figures = {}
        while i < len(lines) and not re.match(r'\s*\.(text|section\s+\.text)', lines[i]) and len(figures) < len(FIGURES):
            for key, label in FIGURES:
                f = re.match(r';\s*%s:\s*(\S+)' % label, lines[i])
                if f:
                    figures[key] = f.group(1)
            i += 1
        found[name] = ('\n'.join(body) + '\n', figures)
    missing = names - set(found)
    if missing:
        sys.exit('isa_digest: no code found for %s' % ', '.join(sorted(missing)))
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('files', nargs='*', help='.hip files (default: %s of xfr_amd/csrc)' % ', '.join(DEFAULT_FILES))
    ap.add_argument('--dump', metavar='DIR', help='write the normalised text of every kernel to DIR/<file>/<kernel>.s')
    args = ap.parse_args()
    files = [os.path.abspath(f) for f in args.files] or [os.path.join(CSRC, f) for f in DEFAULT_FILES]
    total = hashlib.sha256()
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(len(files)) as pool:
        for path, asm in zip(files, pool.map(lambda f: compile_asm(f, tmp), files)):
            base = os.path.basename(path)
            kernels = kernels_of(asm)
            for name in sorted(kernels):
                text, fig = kernels[name]
                line = '%s  %s  %s  %s' % (hashlib.sha256(text.encode()).hexdigest(), base, name, ' '.join('%s=%s' % (k, fig.get(k, '?')) for k, _ in FIGURES))
                if args.dump:
                    os.makedirs(os.path.join(args.dump, base), exist_ok=True)
                    stem = '%s_%s' % (name[:160], hashlib.sha256(name.encode()).hexdigest()[:8])      # mangled names outgrow a file name
                    open(os.path.join(args.dump, base, stem + '.s'), 'w').write(text)
                total.update(line.encode() + b'\n')
                print(line)
            print('# %s: %d kernels' % (base, len(kernels)))
    print('%s  total' % total.hexdigest())


if __name__ == '__main__':
    main()
