"""The torchvision ResNet family (torchvision/models/resnet.py) for the EBP hot path, with torchvision's state-dict names: BasicBlock nets
(resnet18 [2,2,2,2], resnet34 [3,4,6,3]) and Bottleneck v1.5 nets (resnet50 [3,4,6,3]: the stride on the 3x3), functional `out += identity`,
in-place ReLU, a 1x1 / stride 2 projection + BatchNorm shortcut where a stage opens.  The strided 3x3 layers behind the stem run their
backward-data pass by phases (xfr_amd/csrc/plan.hip).  `groups` and `width_per_group` are torchvision's: the Bottleneck's inner width is
int(planes * width_per_group / 64) * groups and its 3x3 (conv2) is a grouped convolution (xfr_amd/csrc/conv_group.hip) -- ResNeXt-50 32x4d,
ResNeXt-101 32x8d and 64x4d; width_per_group = 128 alone gives wide_resnet50_2.

`width` is the channel count of the first stage (64 in torchvision), `in_shape` any C x H x W whose last stage map is square: the
AdaptiveAvgPool2d((1, 1)) in front of `fc` is an average pool over that map."""
import torch

from ..program import Program
from ._backbone import Backbone


class TVResnet(Backbone):
    arch = 'tv_resnet'

    def __init__(self, block='basic', layers=(2, 2, 2, 2), num_classes=1000, width=64, in_shape=(3, 224, 224), groups=1, width_per_group=64):
        super(TVResnet, self).__init__()
        if block not in ('basic', 'bottleneck'):
            raise ValueError("block must be 'basic' or 'bottleneck'")
        if block == 'basic' and (groups != 1 or width_per_group != 64):
            raise ValueError('BasicBlock only supports groups=1 and base_width=64')
        self.groups = int(groups)
        self.width_per_group = int(width_per_group)
        self.block = block
        self.layers = tuple(int(v) for v in layers)
        self.num_classes = int(num_classes)
        self.width = int(width)
        self.in_shape = tuple(int(v) for v in in_shape)
        self.expansion = 1 if block == 'basic' else 4
        self.meta = {'mean': [0.485, 0.456, 0.406], 'std': [0.229, 0.224, 0.225], 'imageSize': [self.in_shape[1], self.in_shape[2], self.in_shape[0]]}
        self.init_parameters()

    def _blocks(self):
        """(prefix, input channels, planes, stride, has a projection shortcut) per block, torchvision's _make_layer."""
        cin = self.width
        for s, nblocks in enumerate(self.layers):
            planes = self.width << s
            for b in range(nblocks):
                stride = 2 if (b == 0 and s > 0) else 1
                yield 'layer%d.%d' % (s + 1, b), cin, planes, stride, (stride != 1 or cin != planes * self.expansion)
                cin = planes * self.expansion

    def inner_width(self, planes):
        """torchvision's Bottleneck: width = int(planes * (base_width / 64.0)) * groups."""
        return int(planes * (self.width_per_group / 64.0)) * self.groups

    @property
    def feature_dim(self):
        return (self.width << (len(self.layers) - 1)) * self.expansion

    def param_specs(self):
        specs = []

        def conv(p, cin, cout, k, groups=1):
            specs.append((p + '.weight', (cout, cin // groups, k, k), 'conv_w'))

        def bn(p, c):
            specs.extend([(p + '.weight', (c,), 'bn_w'), (p + '.bias', (c,), 'bn_b'),
                          (p + '.running_mean', (c,), 'bn_mean'), (p + '.running_var', (c,), 'bn_var'),
                          (p + '.num_batches_tracked', (), 'bn_nbt')])
        conv('conv1', self.in_shape[0], self.width, 7)
        bn('bn1', self.width)
        for pre, cin, planes, stride, proj in self._blocks():
            if self.block == 'basic':
                conv(pre + '.conv1', cin, planes, 3)
                bn(pre + '.bn1', planes)
                conv(pre + '.conv2', planes, planes, 3)
                bn(pre + '.bn2', planes)
            else:
                wd = self.inner_width(planes)
                conv(pre + '.conv1', cin, wd, 1)
                bn(pre + '.bn1', wd)
                conv(pre + '.conv2', wd, wd, 3, self.groups)
                bn(pre + '.bn2', wd)
                conv(pre + '.conv3', wd, planes * 4, 1)
                bn(pre + '.bn3', planes * 4)
            if proj:
                conv(pre + '.downsample.0', cin, planes * self.expansion, 1)
                bn(pre + '.downsample.1', planes * self.expansion)
        specs.append(('fc.weight', (self.num_classes, self.feature_dim), 'fc_w'))
        specs.append(('fc.bias', (self.num_classes,), 'fc_b'))
        return specs

    def build_program(self):
        p = Program(self.in_shape)
        self.forward_on(p)
        p.reprs[p.marks['encode'] - 1] = 'AdaptiveAvgPool2d(output_size=(1, 1))'       # the op that produces tensor t is op t - 1
        return p

    def forward_on(self, p, classifier=True):
        """ResNet._forward_impl, BasicBlock.forward and Bottleneck.forward of torchvision/models/resnet.py, in call order, on any builder with
        the signature of `Program` (the layer program here; the CPU oracle's tape in the tests).  Returns the classify tensor, or with
        classifier=False the pooled features, `fc` not called (the forward under an un-hooked triplet classifier)."""
        h, w = self.in_shape[1:]
        t = p.conv(0, 'conv1', self.width, 7, stride=2, pad=3, bias=False)
        t = p.relu_(p.batchnorm(t, 'bn1'))
        t = p.maxpool(t, 3, 2, 1)
        h, w = ((h + 6 - 7) // 2 + 1 + 2 - 3) // 2 + 1, ((w + 6 - 7) // 2 + 1 + 2 - 3) // 2 + 1
        for pre, cin, planes, stride, proj in self._blocks():
            block_in = t
            if self.block == 'basic':
                o = p.conv(t, pre + '.conv1', planes, 3, stride=stride, pad=1, bias=False)
                o = p.relu_(p.batchnorm(o, pre + '.bn1'))
                o = p.conv(o, pre + '.conv2', planes, 3, stride=1, pad=1, bias=False)
                o = p.batchnorm(o, pre + '.bn2')
            else:
                wd = self.inner_width(planes)
                grouped = dict(groups=self.groups) if self.groups > 1 else {}                   # (builders without grouped layers keep the old signature)
                o = p.conv(t, pre + '.conv1', wd, 1, bias=False)
                o = p.relu_(p.batchnorm(o, pre + '.bn1'))
                o = p.conv(o, pre + '.conv2', wd, 3, stride=stride, pad=1, bias=False, **grouped)      # v1.5: the stride sits on the 3x3
                o = p.relu_(p.batchnorm(o, pre + '.bn2'))
                o = p.conv(o, pre + '.conv3', planes * 4, 1, bias=False)
                o = p.batchnorm(o, pre + '.bn3')
            if proj:
                sc = p.conv(block_in, pre + '.downsample.0', planes * self.expansion, 1, stride=stride, bias=False)
                sc = p.batchnorm(sc, pre + '.downsample.1')
            else:
                sc = block_in
            t = p.relu_(p.g_add(o, sc))                                                        # out += identity; out = self.relu(out)
            if stride == 2:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        if h != w:
            raise ValueError('tv_resnet: the last stage map is %d x %d; the global average pool needs a square map' % (h, w))
        t = p.avgpool(t, h, 1)                                                                 # AdaptiveAvgPool2d((1, 1)) on a fixed input size
        p.mark('encode', t)                                                                    # torch.flatten(x, 1): the pooled features
        if not classifier:
            return t
        return p.mark('classify', p.linear(t, 'fc', self.num_classes, (1, 1), bias=True))


def _make(block, layers, weights_path, kwargs):
    model = TVResnet(block, layers, **kwargs)
    if weights_path:
        model.load_state_dict(torch.load(weights_path, map_location='cpu'))
    return model


def resnet18(weights_path=None, **kwargs):
    return _make('basic', (2, 2, 2, 2), weights_path, kwargs)


def resnet34(weights_path=None, **kwargs):
    return _make('basic', (3, 4, 6, 3), weights_path, kwargs)


def resnet50(weights_path=None, **kwargs):
    """Bottleneck v1.5 [3, 4, 6, 3]."""
    return _make('bottleneck', (3, 4, 6, 3), weights_path, kwargs)


def resnext50_32x4d(weights_path=None, **kwargs):
    return _make('bottleneck', (3, 4, 6, 3), weights_path, dict(kwargs, groups=32, width_per_group=4))


def resnext101_32x8d(weights_path=None, **kwargs):
    return _make('bottleneck', (3, 4, 23, 3), weights_path, dict(kwargs, groups=32, width_per_group=8))


def resnext101_64x4d(weights_path=None, **kwargs):
    return _make('bottleneck', (3, 4, 23, 3), weights_path, dict(kwargs, groups=64, width_per_group=4))


def wide_resnet50_2(weights_path=None, **kwargs):
    """Bottleneck [3, 4, 6, 3] with inner widths twice ResNet-50's (width_per_group = 128); no grouped layer."""
    return _make('bottleneck', (3, 4, 6, 3), weights_path, dict(kwargs, width_per_group=128))
