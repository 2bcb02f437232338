"""MobileNetV1 (Howard et al. 2017, "MobileNets: Efficient Convolutional Neural Networks for Mobile Vision Applications") for the EBP hot path: a
3x3 / stride 2 stem to 32 alpha channels, thirteen depthwise-separable pairs -- depthwise 3x3 + BatchNorm + ReLU, pointwise 1x1 + BatchNorm + ReLU --
of widths 64, 128, 128, 256, 256, 512 x 6, 1024, 1024 (each times alpha) and strides 1, 2, 1, 2, 1, 2, 1 x 5, 2, 1 on the depthwise layer, a global
average pool and `fc`.  The depthwise layers are grouped convolutions with groups = channels (xfr_amd/csrc/conv_depthwise.hip), the strided ones run
their backward-data pass by phases, the pointwise layers are the dense 1x1 GEMMs.  Plain nn.ReLU(inplace=True) throughout (no ReLU6).

head='gdc' replaces the pool by the global depthwise convolution of mobile face networks: a depthwise convolution whose kernel is the last map
(7 x 7 at 224 x 224, 4 x 4 at 112 x 112), pad 0, no ReLU, plus BatchNorm; `fc` then maps the
channels to the embedding.

State-dict names (there is no torchvision MobileNetV1 to follow; these are the attribute paths of the plain-torch statement in
tests/test_depthwise_plan.py): conv1.weight, bn1.*; for pair i = 0 .. 12: blocks.i.dw.weight (C, 1, 3, 3), blocks.i.dw_bn.*, blocks.i.pw.weight
(C', C, 1, 1), blocks.i.pw_bn.*; with head='gdc': gdc.weight (C, 1, h, w), gdc_bn.*; fc.weight, fc.bias.  No convolution has a bias.

`pairs` replaces the thirteen (width, stride) pairs by a shorter or longer list (a truncated trunk for tests and small inputs).
`in_shape` is any C x H x W; with head='avgpool' the last map must be square (the pool is an average pool over that map)."""
import torch

from ..program import Program
from ._backbone import Backbone

WIDTHS = (64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 512, 1024, 1024)
STRIDES = (1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1)


class MobileNetV1(Backbone):
    arch = 'mobilenet_v1'

    def __init__(self, num_classes=1000, alpha=1.0, in_shape=(3, 224, 224), head='avgpool', pairs=None):
        super(MobileNetV1, self).__init__()
        if head not in ('avgpool', 'gdc'):
            raise ValueError("head must be 'avgpool' or 'gdc'")
        self.num_classes = int(num_classes)
        self.alpha = float(alpha)
        self.head = head
        self.in_shape = tuple(int(v) for v in in_shape)
        self.pairs = tuple((int(c), int(s)) for c, s in (pairs if pairs is not None else zip(WIDTHS, STRIDES)))
        self.stem = self._c(32)
        if self.stem < 1:
            raise ValueError('alpha %g leaves no channel' % alpha)
        self.meta = {'mean': [0.485, 0.456, 0.406], 'std': [0.229, 0.224, 0.225], 'imageSize': [self.in_shape[1], self.in_shape[2], self.in_shape[0]]}
        self.init_parameters()

    def _c(self, c):
        return int(c * self.alpha)

    def _pairs(self):
        """(prefix, input channels, output channels, stride of the depthwise layer) per depthwise-separable pair."""
        cin = self.stem
        for i, (c, s) in enumerate(self.pairs):
            yield 'blocks.%d' % i, cin, self._c(c), s
            cin = self._c(c)

    def last_map(self):
        """(h, w) of the last pair's output."""
        h, w = self.in_shape[1:]
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1              # 3x3 / stride 2 / pad 1
        for _, s in self.pairs:
            if s == 2:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        return h, w

    @property
    def feature_dim(self):
        return self._c(self.pairs[-1][0])

    def param_specs(self):
        specs = []

        def conv(p, cout, cin, kh, kw):
            specs.append((p + '.weight', (cout, cin, kh, kw), 'conv_w'))

        def bn(p, c):
            specs.extend([(p + '.weight', (c,), 'bn_w'), (p + '.bias', (c,), 'bn_b'),
                          (p + '.running_mean', (c,), 'bn_mean'), (p + '.running_var', (c,), 'bn_var'),
                          (p + '.num_batches_tracked', (), 'bn_nbt')])
        conv('conv1', self.stem, self.in_shape[0], 3, 3)
        bn('bn1', self.stem)
        for pre, cin, cout, _ in self._pairs():
            conv(pre + '.dw', cin, 1, 3, 3)
            bn(pre + '.dw_bn', cin)
            conv(pre + '.pw', cout, cin, 1, 1)
            bn(pre + '.pw_bn', cout)
        if self.head == 'gdc':
            h, w = self.last_map()
            conv('gdc', self.feature_dim, 1, h, w)
            bn('gdc_bn', self.feature_dim)
        specs.append(('fc.weight', (self.num_classes, self.feature_dim), 'fc_w'))
        specs.append(('fc.bias', (self.num_classes,), 'fc_b'))
        return specs

    def build_program(self):
        p = Program(self.in_shape)
        self.forward_on(p)
        if self.head == 'avgpool':
            p.reprs[p.marks['encode'] - 1] = 'AdaptiveAvgPool2d(output_size=(1, 1))'       # the op that produces tensor t is op t - 1
        return p

    def forward_on(self, p, classifier=True):
        """The forward in call order on any builder with the signature of `Program` (the layer program here; the CPU oracle's tape in the tests).
        Returns the classify tensor, or with classifier=False the features, `fc` not called (the forward under an un-hooked triplet classifier)."""
        t = p.conv(0, 'conv1', self.stem, 3, stride=2, pad=1, bias=False)
        t = p.relu_(p.batchnorm(t, 'bn1'))
        for pre, cin, cout, stride in self._pairs():
            t = p.conv(t, pre + '.dw', cin, 3, stride=stride, pad=1, bias=False, groups=cin)
            t = p.relu_(p.batchnorm(t, pre + '.dw_bn'))
            t = p.conv(t, pre + '.pw', cout, 1, bias=False)
            t = p.relu_(p.batchnorm(t, pre + '.pw_bn'))
        h, w = self.last_map()
        if self.head == 'gdc':
            t = p.conv(t, 'gdc', self.feature_dim, h if h == w else (h, w), stride=1, pad=0, bias=False, groups=self.feature_dim)
            t = p.batchnorm(t, 'gdc_bn')
        else:
            if h != w:
                raise ValueError('mobilenet_v1: the last map is %d x %d; the global average pool needs a square map' % (h, w))
            t = p.avgpool(t, h, 1)                                                             # AdaptiveAvgPool2d((1, 1)) on a fixed input size
        p.mark('encode', t)                                                                    # torch.flatten(x, 1): the features
        if not classifier:
            return t
        return p.mark('classify', p.linear(t, 'fc', self.num_classes, (1, 1), bias=True))


def _make(weights_path, kwargs):
    model = MobileNetV1(**kwargs)
    if weights_path:
        model.load_state_dict(torch.load(weights_path, map_location='cpu'))
    return model


def mobilenet_v1(weights_path=None, **kwargs):
    return _make(weights_path, kwargs)


def mobilefacenet_like(weights_path=None, num_classes=128, in_shape=(3, 112, 112), **kwargs):
    """The MobileNetV1 trunk with the global depthwise head of mobile face networks at 112 x 112; `num_classes` is the embedding width."""
    return _make(weights_path, dict(kwargs, num_classes=num_classes, in_shape=in_shape, head='gdc'))
