#!/usr/bin/env python
"""What the REAL reference computes for a network with depthwise convolutions: a plain-torch mini MobileNetV1 (stem 3x3 s2 -> 8, depthwise 3x3 s1,
pointwise -> 16, depthwise 3x3 s2, pointwise -> 32, each with BatchNorm + ReLU, a global depthwise convolution over the 10 x 9 map + BatchNorm, fc;
input 3 x 40 x 36) wrapped in a subclass of the reference's WhiteboxNetwork.  Conv2d(groups = C) is a module with a .weight, so the reference's
hooks treat it like any other convolution.  Needs the reference checkout (ref_import.py):
    python tests/golden/make_golden_depthwise.py   ->   tests/golden/golden_depthwise.npz
Per subtree mode (affineonly_with_prior, norelu): `ebp` on the hooked classifier (class 3) and the triplet `contrastive_ebp` -- the per-firing
P sums, class names and full layer names (str(module): `groups=` shows there), the pooled P[-2] and the final map.  Arrays and name lists only.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

import ref_import  # noqa: E402
import depthwise_golden_inputs as G  # noqa: E402


class Pair(nn.Sequential):
    """A depthwise-separable pair; the attribute names are the state-dict names of xfr_amd/models/mobilenet.py."""

    def __init__(self, cin, cout, stride):
        super(Pair, self).__init__()
        self.dw = nn.Conv2d(cin, cin, 3, stride=stride, padding=1, groups=cin, bias=False)
        self.dw_bn = nn.BatchNorm2d(cin)
        self.dw_relu = nn.ReLU(inplace=True)
        self.pw = nn.Conv2d(cin, cout, 1, bias=False)
        self.pw_bn = nn.BatchNorm2d(cout)
        self.pw_relu = nn.ReLU(inplace=True)


class MiniMobileNet(nn.Module):
    def __init__(self, num_classes=7):
        super(MiniMobileNet, self).__init__()
        self.conv1 = nn.Conv2d(3, 8, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(8)
        self.relu = nn.ReLU(inplace=True)
        self.blocks = nn.Sequential(Pair(8, 16, 1), Pair(16, 32, 2))
        self.gdc = nn.Conv2d(32, 32, G.LAST_MAP, groups=32, bias=False)
        self.gdc_bn = nn.BatchNorm2d(32)
        self.fc = nn.Linear(32, num_classes)

    def features(self, x):
        x = self.blocks(self.relu(self.bn1(self.conv1(x))))
        return torch.flatten(self.gdc_bn(self.gdc(x)), 1)

    def forward(self, x):
        f = self.features(x)
        return self.fc2(f) if 'fc2' in self._modules else self.fc(f)


def compute():
    """Every array of the golden, from the live reference."""
    ns = ref_import.load()
    torch.set_num_threads(8)

    class WhiteboxMini(ns.whitebox.WhiteboxNetwork):
        def set_triplet_classifier(self, x_mate, x_nonmate):
            self.net.fc2 = nn.Linear(x_mate.shape[1], 2, bias=False)
            self.net.fc2.weight = nn.Parameter(torch.cat((x_mate, x_nonmate), dim=0))

        def encode(self, x):
            return self.net.features(x)

        def classify(self, x):
            return self.net(x)

        def num_classes(self):
            return self.net.fc2.out_features if 'fc2' in self.net._modules else self.net.fc.out_features

    _, sd = G.mini_backbone()
    x = G.image()
    xm, xn = G.triplet_rows()
    out = {}
    for mode in G.MODES:
        net = MiniMobileNet(G.NUM_CLASSES)
        net.load_state_dict(sd, strict=True)
        net.eval()
        wbn = WhiteboxMini(net)
        wb = ns.whitebox.Whitebox(wbn, ebp_subtree_mode=mode)
        out['%s/ebp/map' % mode] = wb.ebp(x, G.class_seed(3, G.NUM_CLASSES))
        out['%s/ebp/names' % mode] = np.array([n.split('(')[0] for n in wb.P_layername])
        out['%s/ebp/layernames' % mode] = np.array([str(n) for n in wb.P_layername])
        out['%s/ebp/sums' % mode] = np.array([float(p.detach().double().sum()) for p in wb.P])
        out['%s/ebp/pooled' % mode] = np.squeeze(np.sum(wb.P[-2].detach().numpy(), axis=1)).astype(np.float32)
        wbn.set_triplet_classifier(xm, xn)
        out['%s/triplet/map' % mode] = wb.contrastive_ebp(x, 0, 1)
        out['%s/triplet/names' % mode] = np.array([n.split('(')[0] for n in wb.P_layername])
        out['%s/triplet/sums' % mode] = np.array([float(p.detach().double().sum()) for p in wb.P])            # the non-mate sweep: the last one run
        out['%s/triplet/pooled' % mode] = np.squeeze(np.sum(wb.P[-2].detach().numpy(), axis=1)).astype(np.float32)
    for k, v in out.items():
        if v.dtype.kind == 'f':
            assert np.isfinite(v).all(), k
    return out


def main():
    out = compute()
    np.savez_compressed(os.path.join(HERE, G.GOLDEN), **out)
    print({k: (v.shape, float(np.abs(v).max()) if v.dtype.kind == 'f' else '') for k, v in out.items()})


if __name__ == '__main__':
    main()
