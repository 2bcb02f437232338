#!/usr/bin/env python
"""What the REAL reference computes for a network with grouped convolutions: a plain-torch mini ResNeXt (torchvision's Bottleneck [1, 1, 1, 1],
width 16, groups 4, width_per_group 16, input 3 x 40 x 36) wrapped in a subclass of the reference's WhiteboxNetwork.  Conv2d(groups = 4) is a
module with a .weight, so the reference's hooks treat it like any other convolution.  Needs the reference checkout (ref_import.py):
    python tests/golden/make_golden_grouped.py   ->   tests/golden/golden_grouped.npz
Per subtree mode (affineonly_with_prior, norelu): `ebp` on the hooked classifier (class 3) and the triplet `contrastive_ebp` -- the per-firing
P sums, class names and full layer names (str(module): `groups=4` shows there), the pooled P[-2] and the final map.  Arrays and name lists only.
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
import grouped_golden_inputs as G  # noqa: E402


class Bottleneck(nn.Sequential):
    """torchvision's Bottleneck (v1.5, groups and base_width).  A Sequential by type only, so that the reference's layer visitor (whitebox.py:42)
    descends into it and hooks its leaves; the forward is torchvision's."""

    def __init__(self, cin, planes, stride=1, downsample=None, groups=1, base_width=64):
        super(Bottleneck, self).__init__()
        width = int(planes * (base_width / 64.0)) * groups
        self.conv1 = nn.Conv2d(cin, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        if downsample is not None:
            self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if 'downsample' in self._modules:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


class MiniResNeXt(nn.Module):
    """torchvision's ResNet(Bottleneck, [1, 1, 1, 1], groups=4, width_per_group=16) at width 16."""

    def __init__(self, width=16, num_classes=7, groups=4, base_width=16):
        super(MiniResNeXt, self).__init__()
        self.conv1 = nn.Conv2d(3, width, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        cin = width
        for s in range(4):
            planes = width << s
            stride = 1 if s == 0 else 2
            down = None
            if stride != 1 or cin != planes * 4:
                down = nn.Sequential(nn.Conv2d(cin, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
            setattr(self, 'layer%d' % (s + 1), nn.Sequential(Bottleneck(cin, planes, stride, down, groups, base_width)))
            cin = planes * 4
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(cin, num_classes)

    def features(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return torch.flatten(self.avgpool(x), 1)

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
        net = MiniResNeXt(16, G.NUM_CLASSES, G.GROUPS, 16)
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
