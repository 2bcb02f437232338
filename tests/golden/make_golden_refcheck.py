#!/usr/bin/env python
"""What the REAL reference computes for the cases of tests/test_oracle_vs_reference.py, so that those checks run without it.
Needs the reference checkout (ref_import.py):   python tests/golden/make_golden_refcheck.py   ->   tests/golden/golden_refcheck.npz

One sweep of the [1,1,1,1] STR-ResNet at 224 x 224 leaves 60 P tensors of 14.7 M floats (59 MB), too large to commit.  Per P tensor the
fixture holds what the test's element-wise bound (max|oracle - reference| <= 1e-6 max|reference|) can be checked against without the tensor
itself (refcheck_summary): its shape, max|P|, sum, sum of squares, a seeded +-1-weighted sum, and the values at the position of max|P| and at 128
seeded positions.  The uint8 saliency map of the ebp_version-5 case is stored whole.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

import ref_import  # noqa: E402
from golden_cases import refcheck_summary  # noqa: E402
from parity_utils import make_backbone, make_images  # noqa: E402
from xfr_amd import synth  # noqa: E402

MODES = ('affineonly_with_prior', 'norelu', 'all', 'affineonly')


def ref_whitebox(ns, recipe, **kw):
    bb, sd = make_backbone('stresnet_mini', seed=9, recipe=recipe, num_classes=5)
    net = ns.resnet.ResNet(ns.resnet.Bottleneck, [1, 1, 1, 1], mode='encode', num_classes=5)
    net.load_state_dict(sd, strict=True)
    net.eval()
    wbn = ns.whitebox.WhiteboxSTResnet(net)
    return wbn, ns.whitebox.Whitebox(wbn, **kw)


def put(out, key, wb):
    out[key + '/names'] = np.array([n.split('(')[0] for n in wb.P_layername])
    for k, v in refcheck_summary([p.detach() for p in wb.P]).items():
        out[key + '/' + k] = v
    wb._ebp_mode = 'disable'           # as the live comparison left it between its reference and oracle sweeps


def main():
    ns = ref_import.load()
    torch.set_num_threads(8)
    out = {}
    x = make_images('stresnet_mini', 1, seed=11)
    xm, xn = synth.unit_rows(1, 512, seed=1) / 2500, synth.unit_rows(1, 512, seed=2) / 2500
    for mode in MODES:
        wbn, wb = ref_whitebox(ns, 'harsh', ebp_subtree_mode=mode)
        for triplet in (False, True):
            if triplet:
                wbn.set_triplet_classifier(xm, xn)
            Pn = torch.zeros(1, 2 if triplet else 5)
            Pn[0, 1] = 1
            wb.ebp(x, Pn, mwp=True)
            put(out, 'P/%s/%s' % (mode, 'triplet' if triplet else 'hooked'), wb)
    _, wb = ref_whitebox(ns, 'mild', ebp_subtree_mode='all', with_bias=True)
    Pn = torch.zeros(1, 5)
    Pn[0, 3] = 1
    wb.ebp(x, Pn, mwp=True)
    put(out, 'P/with_bias', wb)
    wbn, wb = ref_whitebox(ns, 'mild', ebp_version=5)
    wbn.set_triplet_classifier(xm, xn)
    out['uint8_map'] = wb.contrastive_ebp(x, 0, 1)
    np.savez_compressed(os.path.join(HERE, 'golden_refcheck.npz'), **out)
    print({k: v.shape for k, v in out.items() if not k.endswith('/names')})


if __name__ == '__main__':
    main()
