"""Plain-torch fp32 restatement of the reference EfficientNet-Lite backbones (torchok/models/backbones/efficientnet.py:506-575,
:890-928, :1528-1569 on [timm 0.6.13] efficientnet_builder / efficientnet_blocks): the oracle of tests/test_efficientnet_lite*.py.
No squeeze-excite; the stem, every block and the head activate with nn.ReLU6; depthwise convolutions are nn.Conv2d(groups=c),
BatchNorm is nn.BatchNorm2d, module names are timm's, so state_dicts load both ways.  The stage depths follow timm's depth
multiplier rule, restated in `scaled_repeats`.  It lives under tests/ because oracle/ is frozen."""
import math

import torch.nn as nn

from mobilenetv3_ref import dist, grad_scale, make_divisible  # noqa: F401  (the step tests measure with the same two helpers)

# (block type, repeats, kernel, stride, expansion, channels) of the seven stages
ARCH = [('ds', 1, 3, 1, 1, 16), ('ir', 2, 3, 2, 6, 24), ('ir', 2, 5, 2, 6, 40), ('ir', 3, 3, 2, 6, 80), ('ir', 3, 5, 1, 6, 112),
        ('ir', 4, 5, 2, 6, 192), ('ir', 1, 3, 1, 6, 320)]
# name -> (channel multiplier, depth multiplier)
NAMES = {'efficientnet_lite0': (1.0, 1.0), 'efficientnet_lite1': (1.0, 1.1), 'efficientnet_lite2': (1.1, 1.2),
         'efficientnet_lite3': (1.2, 1.4), 'efficientnet_lite4': (1.4, 1.8)}
STEM, HEAD = 32, 1280


def scaled_repeats(repeats, multiplier):
    """One stage: the total ceil(sum(repeats) * multiplier) handed out from the last entry to the first, each taking
    max(1, round(its share of what is left))."""
    left, left_scaled = sum(repeats), int(math.ceil(sum(repeats) * multiplier))
    out = []
    for r in repeats[::-1]:
        rs = max(1, round(r / left * left_scaled))
        out.insert(0, rs)
        left, left_scaled = left - r, left_scaled - rs
    return out


def stage_depths(name):
    """blocks per stage: the first and the last stage keep their depth (fix_first_last)"""
    mult = NAMES[name][1]
    return [r if i in (0, len(ARCH) - 1) else scaled_repeats([r], mult)[0] for i, (_, r, *_) in enumerate(ARCH)]


def stage_widths(name):
    return [make_divisible(c * NAMES[name][0]) for *_, c in ARCH]


class DepthwiseSeparableConv(nn.Module):
    def __init__(self, cin, cout, k, stride):
        super().__init__()
        self.has_skip = stride == 1 and cin == cout
        self.conv_dw = nn.Conv2d(cin, cin, k, stride, k // 2, groups=cin, bias=False)
        self.bn1 = nn.BatchNorm2d(cin)
        self.conv_pw = nn.Conv2d(cin, cout, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.act = nn.ReLU6()

    def forward(self, x):
        y = self.bn2(self.conv_pw(self.act(self.bn1(self.conv_dw(x)))))
        return y + x if self.has_skip else y


class InvertedResidual(nn.Module):
    def __init__(self, cin, cout, k, stride, exp):
        super().__init__()
        mid = make_divisible(cin * exp)
        self.has_skip = stride == 1 and cin == cout
        self.conv_pw = nn.Conv2d(cin, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv_dw = nn.Conv2d(mid, mid, k, stride, k // 2, groups=mid, bias=False)
        self.bn2 = nn.BatchNorm2d(mid)
        self.conv_pwl = nn.Conv2d(mid, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)
        self.act = nn.ReLU6()

    def forward(self, x):
        y = self.act(self.bn1(self.conv_pw(x)))
        y = self.act(self.bn2(self.conv_dw(y)))
        y = self.bn3(self.conv_pwl(y))
        return y + x if self.has_skip else y


class EfficientNetLite(nn.Module):
    def __init__(self, name, in_channels=3):
        super().__init__()
        depths, widths = stage_depths(name), stage_widths(name)
        cin = STEM                                          # fix_stem: not scaled by the channel multiplier
        self.conv_stem = nn.Conv2d(in_channels, cin, 3, 2, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cin)
        stages, self.features = [], []
        for si, ((bt, _, k, s, e, _), depth, cout) in enumerate(zip(ARCH, depths, widths)):
            blocks = []
            for i in range(depth):
                stride = s if i == 0 else 1
                blocks.append(DepthwiseSeparableConv(cin, cout, k, stride) if bt == 'ds' else
                              InvertedResidual(cin, cout, k, stride, e))
                cin = cout
            if si + 1 == len(ARCH) or ARCH[si + 1][3] > 1:
                self.features.append(f'blocks.{si}.{depth - 1}')
            stages.append(nn.Sequential(*blocks))
        self.blocks = nn.Sequential(*stages)
        self.conv_head = nn.Conv2d(cin, HEAD, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(HEAD)
        self.act = nn.ReLU6()
        self.out_channels = HEAD
        for m in self.modules():                            # [timm] _init_weight_goog
            if isinstance(m, nn.Conv2d):
                fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
                m.weight.data.normal_(0, math.sqrt(2.0 / fan_out))

    def forward(self, x):
        x = self.act(self.bn1(self.conv_stem(x)))
        x = self.blocks(x)
        return self.act(self.bn2(self.conv_head(x)))

    def forward_features(self, x):
        feats = [x]
        x = self.act(self.bn1(self.conv_stem(x)))
        for si, stage in enumerate(self.blocks):
            for bi, block in enumerate(stage):
                x = block(x)
                if f'blocks.{si}.{bi}' in self.features:
                    feats.append(x)
        return feats


class Classifier(nn.Module):
    """backbone -> global average pool -> head.fc: the children of ClassificationTask with Pooling + ClassificationHead
    (the interface oracle.torchok_ref.training_step drives)."""

    def __init__(self, name, num_classes):
        super().__init__()
        self.backbone = EfficientNetLite(name)
        self.head = nn.Module()
        self.head.fc = nn.Linear(self.backbone.out_channels, num_classes)

    def forward_with_gt(self, batch):
        emb = self.backbone(batch['image']).mean((2, 3))
        return {'embeddings': emb, 'prediction': self.head.fc(emb), 'target': batch['target']}
