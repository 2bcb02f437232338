"""The inputs of the grouped-network golden (tests/golden/golden_grouped.npz), shared by the script that makes it from the live reference
(tests/golden/make_golden_grouped.py) and by the tests that hold the oracle tape and the engine to it: a mini ResNeXt (Bottleneck [1, 1, 1, 1],
width 16, groups 4, width_per_group 16, 3 x 40 x 36 input, 7 classes) with seeded weights, the image and the class seeds of
tests/strided_golden_inputs.py, seeded triplet rows."""
import numpy as np
import torch

import layer_nets as L
from oracle import ebp_oracle as O
from strided_golden_inputs import IN_SHAPE, MODES, NUM_CLASSES, class_seed, image  # noqa: F401
from xfr_amd import synth
from xfr_amd.models import tv_resnet

GOLDEN = 'golden_grouped.npz'
GROUPS = 4
FEATURES = 16 * 8 * 4


def mini_backbone():
    bb = tv_resnet.TVResnet('bottleneck', (1, 1, 1, 1), num_classes=NUM_CLASSES, width=16, in_shape=IN_SHAPE, groups=GROUPS, width_per_group=16)
    sd = synth.synth_state_dict(bb, seed=27, recipe='mild')
    bb.load_state_dict(sd)
    return bb, sd


def triplet_rows():
    return synth.unit_rows(1, FEATURES, seed=1) / 50, synth.unit_rows(1, FEATURES, seed=2) / 50


class OracleTVResnext(object):
    """ebp and contrastive_ebp of whitebox.py:482-527 for the mini net on the oracle tape (the grouped builder of tests/grouped_nets.py under
    tv_resnet.forward_on), the hooked `fc` or the un-hooked triplet classifier."""

    def __init__(self, bb, sd, mode, dtype=torch.float32):
        self.bb, self.sd, self.mode, self.dtype = bb, sd, mode, dtype
        self.triplet = None

    def set_triplet_classifier(self, x_mate, x_nonmate):
        self.triplet = torch.cat((x_mate, x_nonmate), dim=0)

    def ebp(self, x, Pn):
        """-> (P list, pooled P[-2])"""
        tape = O.Tape({k: v for k, v in self.sd.items() if v.dtype.is_floating_point}, dtype=self.dtype)
        b = L._TapeBuilder(tape, x)
        tape.input(x)
        out = self.bb.forward_on(b, classifier=self.triplet is None)
        if self.triplet is not None:
            out = tape.g_linear(tape.g_flatten(out), self.triplet)
        P, _ = tape.backward(out, Pn, self.mode, 1e-16)
        return P, np.squeeze(np.sum(P[-2].detach().numpy(), axis=1)).astype(np.float32)

    def contrastive_ebp(self, x, k_pos, k_neg):
        n = 2 if self.triplet is not None else NUM_CLASSES
        Pm, _ = self.ebp(x, class_seed(k_pos, n))
        Pq, _ = self.ebp(x, class_seed(k_neg, n))
        m, q = Pm[-2] / torch.sum(Pm[-2]), Pq[-2] / torch.sum(Pq[-2])
        c = np.squeeze(np.sum(torch.relu(m - q).numpy(), axis=1).astype(np.float32))
        return O.mwp_to_saliency(c)
