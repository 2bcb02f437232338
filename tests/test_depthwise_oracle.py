"""The depthwise-network golden (tests/golden/golden_depthwise.npz: a mini MobileNetV1 with a global depthwise head through the live reference)
without a GPU: the CPU oracle's tape, driven by the forward of xfr_amd/models/mobilenet.py, reproduces every recorded firing, pooled map and final
map, and the layer program prints the reference's layer names (`groups=` in them); and where the reference checkout is present, the live reference
still produces the file."""
import os
import sys

import numpy as np
import pytest

import depthwise_golden_inputs as G
from parity_utils import MAP_RTOL_CONTRAST, assert_map_close

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import ref_import  # noqa: E402


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(HERE, 'golden', G.GOLDEN))


@pytest.mark.parametrize('mode', G.MODES)
def test_oracle_tape_matches_reference(golden, mode):
    from oracle import ebp_oracle as O
    bb, sd = G.mini_backbone()
    x = G.image()
    ow = G.OracleMobileNet(bb, sd, mode)
    P, pooled = ow.ebp(x, G.class_seed(3, G.NUM_CLASSES))
    gs, gn = golden['%s/ebp/sums' % mode], golden['%s/ebp/names' % mode]
    assert len(P) == len(gs)
    err = np.abs(np.array([float(p.double().sum()) for p in P]) - gs) / np.maximum(np.abs(gs), 1e-300)
    assert err.max() <= 1e-4, (mode, int(err.argmax()), err.max())
    assert_map_close(pooled, golden['%s/ebp/pooled' % mode], '%s ebp pooled P[-2]' % mode)
    assert_map_close(O.mwp_to_saliency(pooled), golden['%s/ebp/map' % mode], '%s ebp map' % mode)
    # the reference's firing order and its str(module) of every firing: Whitebox.P_layername, `groups=` on the three depthwise layers
    prog = bb.build_program()
    full = prog.layernames(mode, prog.marks['classify'])
    assert [n.split('(')[0] for n in full] == list(gn), (full, list(gn))
    assert full == [str(n) for n in golden['%s/ebp/layernames' % mode]]
    assert sum('groups=' in n for n in full) == 3
    assert 'Conv2d(32, 32, kernel_size=(10, 9), stride=(1, 1), groups=32, bias=False)' in full
    ow.set_triplet_classifier(*G.triplet_rows())
    assert_map_close(ow.contrastive_ebp(x, 0, 1), golden['%s/triplet/map' % mode], '%s triplet map' % mode, rtol=MAP_RTOL_CONTRAST)
    Pq, pooled_q = ow.ebp(x, G.class_seed(1, 2))
    gs = golden['%s/triplet/sums' % mode]
    assert len(Pq) == len(gs)
    err = np.abs(np.array([float(p.double().sum()) for p in Pq]) - gs) / np.maximum(np.abs(gs), 1e-300)
    assert err.max() <= 1e-4, (mode, int(err.argmax()), err.max())
    assert_map_close(pooled_q, golden['%s/triplet/pooled' % mode], '%s triplet pooled P[-2]' % mode)


@pytest.mark.skipif(not ref_import.available(), reason='the reference checkout is not present')
def test_live_reference_still_makes_the_golden(golden):
    import make_golden_depthwise
    live = make_golden_depthwise.compute()
    assert sorted(live) == sorted(golden.files)
    for k in golden.files:
        if golden[k].dtype.kind == 'f':
            assert live[k].shape == golden[k].shape and np.allclose(live[k], golden[k], rtol=1e-5, atol=1e-7 * float(np.abs(golden[k]).max())), k
        else:
            assert list(live[k]) == list(golden[k]), k
