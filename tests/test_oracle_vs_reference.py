"""Cross-check of the oracle against the real reference, P tensor by P tensor, through what the reference computed for the same cases
(tests/golden/make_golden_refcheck.py -> golden_refcheck.npz: per P tensor its shape, max, sums and the values at seeded positions; a
sweep's 59 MB of P tensors are too large to commit)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from golden_cases import check_refcheck, golden  # noqa: E402
from parity_utils import make_backbone, make_images  # noqa: E402
from xfr_amd import synth  # noqa: E402


@pytest.mark.parametrize('mode', ['affineonly_with_prior', 'norelu', 'all', 'affineonly'])
def test_every_P_tensor_matches_reference(mode):
    from oracle import ebp_oracle as O
    gold = golden('golden_refcheck')
    torch.set_num_threads(8)
    bb, sd = make_backbone('stresnet_mini', seed=9, recipe='harsh', num_classes=5)
    ow = O.OracleWhitebox('stresnet_mini', sd, ('hooked', None), mode)
    x = make_images('stresnet_mini', 1, seed=11)
    for triplet in (False, True):
        if triplet:
            xm, xn = synth.unit_rows(1, 512, seed=1) / 2500, synth.unit_rows(1, 512, seed=2) / 2500
            ow.set_triplet_classifier(xm, xn)
        C = 2 if triplet else 5
        Pn = torch.zeros(1, C)
        Pn[0, 1] = 1
        ow.ebp(x, Pn, mwp=True)
        key = 'P/%s/%s' % (mode, 'triplet' if triplet else 'hooked')
        assert list(gold[key + '/names']) == ow.P_layername
        check_refcheck(ow.P, gold, key)


def test_with_bias_matches_reference():
    """ebp_version 11 / with_bias=True: biases (and BatchNorm beta) are rectified in the positive pass (whitebox.py:321-324)."""
    from oracle import ebp_oracle as O
    gold = golden('golden_refcheck')
    torch.set_num_threads(8)
    bb, sd = make_backbone('stresnet_mini', seed=9, recipe='mild', num_classes=5)
    ow = O.OracleWhitebox('stresnet_mini', sd, ('hooked', None), 'all', with_bias=True)
    x = make_images('stresnet_mini', 1, seed=11)
    Pn = torch.zeros(1, 5)
    Pn[0, 3] = 1
    ow.ebp(x, Pn, mwp=True)
    check_refcheck(ow.P, gold, 'P/with_bias')


def test_uint8_saliency_path_matches_reference():
    """ebp_version != 6: _mwp_to_saliency goes through uint8 + PIL GaussianBlur (whitebox.py:451-454)."""
    from oracle import ebp_oracle as O
    gold = golden('golden_refcheck')
    torch.set_num_threads(8)
    bb, sd = make_backbone('stresnet_mini', seed=9, recipe='mild', num_classes=5)
    ow = O.OracleWhitebox('stresnet_mini', sd, ('hooked', None), 'affineonly_with_prior', ebp_version=5)
    xm, xn = synth.unit_rows(1, 512, seed=1) / 2500, synth.unit_rows(1, 512, seed=2) / 2500
    ow.set_triplet_classifier(xm, xn)
    x = make_images('stresnet_mini', 1, seed=11)
    a = gold['uint8_map']
    b = ow.contrastive_ebp(x, 0, 1)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and np.array_equal(a, b)
