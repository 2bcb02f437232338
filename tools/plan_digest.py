#!/usr/bin/env python
"""Digest of everything the planner decides, for checking a planner change to the byte.  Device-free (xfr_plan_describe):

    python tools/plan_digest.py > before.txt      # on the old build
    python tools/plan_digest.py > after.txt       # on the new one; `diff before.txt after.txt` must be empty

One sha256 per case -- every program of tests/test_plan.py's PROGRAMS x subtree mode x mark x epilogue-fusion level x batch, chain step
types included (XFR_DESCRIBE_TYPES) -- and one over all of them.  --dump DIR also writes each case's text, to see what moved.
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
FUSION_LEVELS = (None, 0, 1, 3, 7, 11, 19, 35, 67, 131, 259)      # xfr_engine_set_epilogue_fusion values: the default, then one switch at a time
BATCHES = (1, 3, 32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--dump', metavar='DIR', help='write the text of every case to DIR/<case>.txt')
    args = ap.parse_args()
    from test_plan import MODES, PROGRAMS
    os.environ['XFR_DESCRIBE_TYPES'] = '1'
    total = hashlib.sha256()
    for arch in sorted(PROGRAMS):
        prog = PROGRAMS[arch]
        for mode in MODES:
            for mark in sorted(prog.marks):
                for fusion in FUSION_LEVELS:
                    os.environ.pop('XFR_DESCRIBE_FUSION', None)
                    if fusion is not None:
                        os.environ['XFR_DESCRIBE_FUSION'] = str(fusion)
                    for batch in BATCHES:
                        case = '%s-%s-%s-f%s-b%d' % (arch, mode, mark, fusion, batch)
                        text = prog.describe(mode, prog.marks[mark], batch=batch).encode()
                        if args.dump:
                            os.makedirs(args.dump, exist_ok=True)
                            open(os.path.join(args.dump, case + '.txt'), 'wb').write(text)
                        total.update(case.encode() + b'\n' + text)
                        print('%s  %s' % (hashlib.sha256(text).hexdigest(), case))
    os.environ.pop('XFR_DESCRIBE_FUSION', None)
    print('%s  total' % total.hexdigest())


if __name__ == '__main__':
    main()
