"""Plain-torch fp32 restatement of the reference MobileNetV3 backbones (torchok/models/backbones/mobilenetv3.py:108-311 on
[timm 0.6.13] efficientnet_builder / efficientnet_blocks): the oracle of tests/test_mobilenetv3*.py.  Activations are
nn.Hardswish / nn.ReLU, the squeeze-excite gate is nn.Hardsigmoid, depthwise convolutions are nn.Conv2d(groups=c), BatchNorm
is nn.BatchNorm2d, module names are timm's, so state_dicts load both ways.  It lives under tests/ because oracle/ is frozen."""
import math

import torch.nn as nn

LARGE = [['ds_r1_k3_s1_e1_c16_nre'], ['ir_r1_k3_s2_e4_c24_nre', 'ir_r1_k3_s1_e3_c24_nre'], ['ir_r3_k5_s2_e3_c40_se0.25_nre'],
         ['ir_r1_k3_s2_e6_c80', 'ir_r1_k3_s1_e2.5_c80', 'ir_r2_k3_s1_e2.3_c80'], ['ir_r2_k3_s1_e6_c112_se0.25'],
         ['ir_r3_k5_s2_e6_c160_se0.25'], ['cn_r1_k1_s1_c960']]
SMALL = [['ds_r1_k3_s2_e1_c16_se0.25_nre'], ['ir_r1_k3_s2_e4.5_c24_nre', 'ir_r1_k3_s1_e3.67_c24_nre'],
         ['ir_r1_k5_s2_e4_c40_se0.25', 'ir_r2_k5_s1_e6_c40_se0.25'], ['ir_r2_k5_s1_e3_c48_se0.25'],
         ['ir_r3_k5_s2_e6_c96_se0.25'], ['cn_r1_k1_s1_c576']]
# name -> (arch, channel multiplier, num_features)
NAMES = {'mobilenetv3_large_075': (LARGE, 0.75, 1280), 'mobilenetv3_large_100': (LARGE, 1.0, 1280),
         'mobilenetv3_large_100_miil': (LARGE, 1.0, 1280), 'mobilenetv3_large_100_miil_in21k': (LARGE, 1.0, 1280),
         'mobilenetv3_small_050': (SMALL, 0.5, 1024), 'mobilenetv3_small_075': (SMALL, 0.75, 1024),
         'mobilenetv3_small_100': (SMALL, 1.0, 1024)}


def make_divisible(v, divisor=8):
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new_v + divisor if new_v < 0.9 * v else new_v


def decode(block_str):
    parts = block_str.split('_')
    d = {'type': parts[0], 'noskip': 'noskip' in parts, 'relu': 'nre' in parts, 'e': 1.0, 'se': 0.0, 'r': 1}
    for p in parts[1:]:
        if p.startswith('se'):
            d['se'] = float(p[2:])
        elif p not in ('noskip', 'nre'):
            d[p[0]] = float(p[1:]) if p[0] == 'e' else int(p[1:])
    return d


def _act(relu):
    return nn.ReLU() if relu else nn.Hardswish()


class SqueezeExcite(nn.Module):
    def __init__(self, chs, rd):
        super().__init__()
        self.conv_reduce = nn.Conv2d(chs, rd, 1, bias=True)
        self.act1 = nn.ReLU()
        self.conv_expand = nn.Conv2d(rd, chs, 1, bias=True)
        self.gate = nn.Hardsigmoid()

    def forward(self, x):
        s = x.mean((2, 3), keepdim=True)
        return x * self.gate(self.conv_expand(self.act1(self.conv_reduce(s))))


def _se(chs, ratio):
    return SqueezeExcite(chs, make_divisible(chs * ratio)) if ratio else nn.Identity()     # rd_round_fn=round_channels


class DepthwiseSeparableConv(nn.Module):
    def __init__(self, cin, cout, k, stride, noskip, se_ratio, relu):
        super().__init__()
        self.has_skip = stride == 1 and cin == cout and not noskip
        self.conv_dw = nn.Conv2d(cin, cin, k, stride, k // 2, groups=cin, bias=False)
        self.bn1 = nn.BatchNorm2d(cin)
        self.se = _se(cin, se_ratio)
        self.conv_pw = nn.Conv2d(cin, cout, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.act = _act(relu)

    def forward(self, x):
        y = self.se(self.act(self.bn1(self.conv_dw(x))))
        y = self.bn2(self.conv_pw(y))
        return y + x if self.has_skip else y


class InvertedResidual(nn.Module):
    def __init__(self, cin, cout, k, stride, noskip, exp, se_ratio, relu):
        super().__init__()
        mid = make_divisible(cin * exp)
        self.has_skip = stride == 1 and cin == cout and not noskip
        self.conv_pw = nn.Conv2d(cin, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv_dw = nn.Conv2d(mid, mid, k, stride, k // 2, groups=mid, bias=False)
        self.bn2 = nn.BatchNorm2d(mid)
        self.se = _se(mid, se_ratio)                       # se_from_exp=True: the ratio of the expanded width
        self.conv_pwl = nn.Conv2d(mid, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)
        self.act = _act(relu)

    def forward(self, x):
        y = self.act(self.bn1(self.conv_pw(x)))
        y = self.se(self.act(self.bn2(self.conv_dw(y))))
        y = self.bn3(self.conv_pwl(y))
        return y + x if self.has_skip else y


class ConvBnAct(nn.Module):
    def __init__(self, cin, cout, k, stride, relu):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride, k // 2, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.act = _act(relu)

    def forward(self, x):
        return self.act(self.bn1(self.conv(x)))


def make_block(d, cin, cout, stride):
    if d['type'] == 'ds':
        return DepthwiseSeparableConv(cin, cout, d['k'], stride, d['noskip'], d['se'], d['relu'])
    if d['type'] == 'ir':
        return InvertedResidual(cin, cout, d['k'], stride, d['noskip'], d['e'], d['se'], d['relu'])
    return ConvBnAct(cin, cout, d['k'], stride, d['relu'])


class MobileNetV3(nn.Module):
    def __init__(self, name, in_channels=3):
        super().__init__()
        arch_def, mult, self.num_features = NAMES[name]

        def rc(c):
            return make_divisible(c * mult)
        cin = 16 if mult < 0.75 else rc(16)                # fix_stem
        self.conv_stem = nn.Conv2d(in_channels, cin, 3, 2, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cin)
        self.act1 = nn.Hardswish()
        stages = []
        decoded = [[decode(s) for s in stack] for stack in arch_def]
        self.features = ['act1'] if decoded[0][0]['s'] > 1 else []
        for si, stack in enumerate(decoded):
            blocks = []
            for d in stack:
                for i in range(d['r']):
                    cout = rc(d['c'])
                    blocks.append(make_block(d, cin, cout, d['s'] if i == 0 and d is stack[0] else 1))
                    cin = cout
            if si + 1 == len(decoded) or decoded[si + 1][0]['s'] > 1:
                self.features.append(f'blocks.{si}.{len(blocks) - 1}')
            stages.append(nn.Sequential(*blocks))
        self.blocks = nn.Sequential(*stages)
        self.out_channels = cin                             # the real width of the returned map
        for m in self.modules():                            # [timm] _init_weight_goog
            if isinstance(m, nn.Conv2d):
                fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
                m.weight.data.normal_(0, math.sqrt(2.0 / fan_out))
                if m.bias is not None:
                    m.bias.data.zero_()

    def forward(self, x):
        return self.blocks(self.act1(self.bn1(self.conv_stem(x))))

    def forward_features(self, x):
        feats = [x]
        x = self.act1(self.bn1(self.conv_stem(x)))
        if 'act1' in self.features:
            feats.append(x)
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
        self.backbone = MobileNetV3(name)
        self.head = nn.Module()
        self.head.fc = nn.Linear(self.backbone.out_channels, num_classes)

    def forward_with_gt(self, batch):
        emb = self.backbone(batch['image']).mean((2, 3))
        return {'embeddings': emb, 'prediction': self.head.fc(emb), 'target': batch['target']}


def grad_scale(name, ref_params):
    """What a gradient's distance to the fp32 reference is measured against: the reference gradient's own norm (rel_err),
    except for the bias of a block's last BatchNorm ('ir': bn3, 'ds': bn2).  Every such block output feeds nothing but a 1x1
    convolution followed by a batch-statistics BatchNorm (the next block's expansion, through the skip connections as well, and
    at the end the 'cn' block), which removes a per-channel constant: that gradient is exactly zero (1e-15 of the weight's in
    fp64), what fp32 returns for it is rounding noise, and a ratio to its norm says nothing.  Those are measured against the
    norm of the same BatchNorm's weight gradient instead; bound and factors are unchanged."""
    parts = name.split('.')
    if len(parts) == 6 and parts[1] == 'blocks' and parts[5] == 'bias' and parts[4] in ('bn2', 'bn3'):
        last = 'bn3' if name.replace(parts[4] + '.bias', 'bn3.weight') in ref_params else 'bn2'
        if parts[4] == last:
            return float(ref_params[name[:-len('bias')] + 'weight'].grad.double().norm())
    return float(ref_params[name].grad.double().norm())


def dist(a, b, scale):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).norm() / (scale + 1e-12))
