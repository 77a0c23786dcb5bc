"""Plain-torch fp32 restatement of the reference MnasNet backbones (torchok/models/backbones/efficientnet.py:506-681 on
[timm 0.6.13] efficientnet_builder / efficientnet_blocks): the oracle of tests/test_mnasnet*.py.  Depthwise convolutions are
nn.Conv2d(groups=c), BatchNorm is nn.BatchNorm2d, module names are timm's, so state_dicts load both ways.  It lives under
tests/ because oracle/ is frozen."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

ARCH = {
    'a1': (32, [['ds_r1_k3_s1_e1_c16_noskip'], ['ir_r2_k3_s2_e6_c24'], ['ir_r3_k5_s2_e3_c40_se0.25'], ['ir_r4_k3_s2_e6_c80'],
                ['ir_r2_k3_s1_e6_c112_se0.25'], ['ir_r3_k5_s2_e6_c160_se0.25'], ['ir_r1_k3_s1_e6_c320']]),
    'b1': (32, [['ds_r1_k3_s1_c16_noskip'], ['ir_r3_k3_s2_e3_c24'], ['ir_r3_k5_s2_e3_c40'], ['ir_r3_k5_s2_e6_c80'],
                ['ir_r2_k3_s1_e6_c96'], ['ir_r4_k5_s2_e6_c192'], ['ir_r1_k3_s1_e6_c320_noskip']]),
    'small': (8, [['ds_r1_k3_s1_c8'], ['ir_r1_k3_s2_e3_c16'], ['ir_r2_k3_s2_e6_c16'], ['ir_r4_k5_s2_e6_c32_se0.25'],
                  ['ir_r3_k3_s1_e6_c32_se0.25'], ['ir_r3_k5_s2_e6_c88_se0.25'], ['ir_r1_k3_s1_e6_c144']]),
}
NAMES = {'mnasnet_050': ('b1', 0.5), 'mnasnet_075': ('b1', 0.75), 'mnasnet_100': ('b1', 1.0), 'mnasnet_b1': ('b1', 1.0),
         'mnasnet_140': ('b1', 1.4), 'semnasnet_050': ('a1', 0.5), 'semnasnet_075': ('a1', 0.75),
         'semnasnet_100': ('a1', 1.0), 'mnasnet_a1': ('a1', 1.0), 'semnasnet_140': ('a1', 1.4),
         'mnasnet_small': ('small', 1.0)}


def make_divisible(v, divisor=8):
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new_v + divisor if new_v < 0.9 * v else new_v


def decode(block_str):
    parts = block_str.split('_')
    d = {'type': parts[0], 'noskip': 'noskip' in parts, 'e': 1.0, 'se': 0.0, 'r': 1}
    for p in parts[1:]:
        if p.startswith('se'):
            d['se'] = float(p[2:])
        elif p != 'noskip':
            d[p[0]] = float(p[1:]) if p[0] == 'e' else int(p[1:])
    return d


class SqueezeExcite(nn.Module):
    def __init__(self, chs, rd):
        super().__init__()
        self.conv_reduce = nn.Conv2d(chs, rd, 1, bias=True)
        self.conv_expand = nn.Conv2d(rd, chs, 1, bias=True)

    def forward(self, x):
        s = x.mean((2, 3), keepdim=True)
        return x * torch.sigmoid(self.conv_expand(F.relu(self.conv_reduce(s))))


class DepthwiseSeparableConv(nn.Module):
    def __init__(self, cin, cout, k, stride, noskip, se_ratio):
        super().__init__()
        self.has_skip = stride == 1 and cin == cout and not noskip
        self.conv_dw = nn.Conv2d(cin, cin, k, stride, k // 2, groups=cin, bias=False)
        self.bn1 = nn.BatchNorm2d(cin)
        self.se = SqueezeExcite(cin, round(cin * se_ratio)) if se_ratio else nn.Identity()
        self.conv_pw = nn.Conv2d(cin, cout, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)

    def forward(self, x):
        y = self.se(F.relu(self.bn1(self.conv_dw(x))))
        y = self.bn2(self.conv_pw(y))
        return y + x if self.has_skip else y


class InvertedResidual(nn.Module):
    def __init__(self, cin, cout, k, stride, noskip, exp, se_ratio):
        super().__init__()
        mid = make_divisible(cin * exp)
        self.has_skip = stride == 1 and cin == cout and not noskip
        self.conv_pw = nn.Conv2d(cin, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv_dw = nn.Conv2d(mid, mid, k, stride, k // 2, groups=mid, bias=False)
        self.bn2 = nn.BatchNorm2d(mid)
        self.se = SqueezeExcite(mid, round(mid * se_ratio)) if se_ratio else nn.Identity()
        self.conv_pwl = nn.Conv2d(mid, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)

    def forward(self, x):
        y = F.relu(self.bn1(self.conv_pw(x)))
        y = self.se(F.relu(self.bn2(self.conv_dw(y))))
        y = self.bn3(self.conv_pwl(y))
        return y + x if self.has_skip else y


class MnasNet(nn.Module):
    def __init__(self, name, in_channels=3, num_features=1280):
        super().__init__()
        arch, mult = NAMES[name]
        stem, arch_def = ARCH[arch]

        def rc(c):
            return make_divisible(c * mult)
        cin = rc(stem)
        self.conv_stem = nn.Conv2d(in_channels, cin, 3, 2, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cin)
        stages, self.features = [], []
        decoded = [[decode(s) for s in stack] for stack in arch_def]
        for si, stack in enumerate(decoded):
            blocks = []
            for d in stack:
                for i in range(d['r']):
                    stride = d['s'] if i == 0 else 1
                    cout = rc(d['c'])
                    se = d['se'] / (d['e'] if d['type'] == 'ir' else 1.0)   # se_from_exp=False
                    if d['type'] == 'ds':
                        blocks.append(DepthwiseSeparableConv(cin, cout, d['k'], stride, d['noskip'], se))
                    else:
                        blocks.append(InvertedResidual(cin, cout, d['k'], stride, d['noskip'], d['e'], se))
                    cin = cout
            if si + 1 == len(decoded) or decoded[si + 1][0]['s'] > 1:
                self.features.append(f'blocks.{si}.{len(blocks) - 1}')
            stages.append(nn.Sequential(*blocks))
        self.blocks = nn.Sequential(*stages)
        self.conv_head = nn.Conv2d(cin, num_features, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(num_features)
        self.out_channels = num_features
        for m in self.modules():                        # [timm] _init_weight_goog
            if isinstance(m, nn.Conv2d):
                fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
                m.weight.data.normal_(0, math.sqrt(2.0 / fan_out))
                if m.bias is not None:
                    m.bias.data.zero_()

    def forward(self, x):
        x = F.relu(self.bn1(self.conv_stem(x)))
        x = self.blocks(x)
        return F.relu(self.bn2(self.conv_head(x)))

    def forward_features(self, x):
        feats = [x]
        x = F.relu(self.bn1(self.conv_stem(x)))
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
        self.backbone = MnasNet(name)
        self.head = nn.Module()
        self.head.fc = nn.Linear(self.backbone.out_channels, num_classes)

    def forward_with_gt(self, batch):
        emb = self.backbone(batch['image']).mean((2, 3))
        return {'embeddings': emb, 'prediction': self.head.fc(emb), 'target': batch['target']}
