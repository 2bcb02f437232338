"""The inputs of the strided-network golden (tests/golden/golden_strided.npz), shared by the script that makes it from the live reference
(tests/golden/make_golden_strided.py) and by the tests that hold the oracle tape and the engine to it: a mini torchvision ResNet
(BasicBlock [1, 1, 1, 1], width 16, 3 x 40 x 36 input, 7 classes) with seeded weights, one seeded image, seeded triplet rows."""
import numpy as np
import torch

import layer_nets as L
from oracle import ebp_oracle as O
from xfr_amd import synth
from xfr_amd.models import tv_resnet

IN_SHAPE = (3, 40, 36)
NUM_CLASSES = 7
MODES = ('affineonly_with_prior', 'norelu')
GOLDEN = 'golden_strided.npz'


def mini_backbone():
    bb = tv_resnet.TVResnet('basic', (1, 1, 1, 1), num_classes=NUM_CLASSES, width=16, in_shape=IN_SHAPE)
    sd = synth.synth_state_dict(bb, seed=21, recipe='mild')
    bb.load_state_dict(sd)
    return bb, sd


def image():
    return synth.synth_smooth_images(1, IN_SHAPE, seed=23, mean=(120.0, 110.0, 100.0)) / 64.0


def triplet_rows():
    d = 16 * 8
    return synth.unit_rows(1, d, seed=1) / 50, synth.unit_rows(1, d, seed=2) / 50


def class_seed(k, n_classes):
    Pn = torch.zeros((1, n_classes))
    Pn[0, k] = 1
    return Pn


class OracleTVResnet(object):
    """ebp and contrastive_ebp of whitebox.py:482-527 for the mini net on the oracle tape, the hooked `fc` or the un-hooked triplet classifier."""

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
