"""MnasNet backbones on the MI355X engine.

Mirrors the reference wiring ``torchok/models/backbones/efficientnet.py``: ``EfficientNet`` (:506-575), ``_gen_mnasnet_a1`` /
``_b1`` / ``_small`` (:583-681) and the MnasNet entry points (:1181-1254), with the [timm 0.6.13] ``decode_arch_def``,
``EfficientNetBuilder``, ``DepthwiseSeparableConv``, ``InvertedResidual``, ``SqueezeExcite``, ``round_channels`` and
``_init_weight_goog`` semantics restated here.  Module / parameter names are those of timm, so reference checkpoints load.

Each ``conv -> bn -> act`` group is one engine unit: the 1x1 expansion / projection, the stem and the head run on
``conv_bn_act`` (the projection of a block with a skip connection adds the block input before nothing else: ``relu=False,
shortcut=x``), the depthwise convolution on ``dwconv_bn_act`` and the squeeze-excite on ``squeeze_excite``.  Only what the
MnasNet family needs is built here: ReLU, BatchNorm, 'ds' / 'ir' blocks; the SiLU / ReLU6 families (EfficientNet,
MobileNetV2, FBNet) stay unregistered.  The hard-swish family (MobileNetV3) has its own file, ``mobilenetv3.py``.
"""
import math
import re
from typing import List

import torch
import torch.nn as nn

from ... import engine
from ...constructor import BACKBONES
from ...engine import functional as EF
from ..base import BaseBackbone


def make_divisible(v, divisor=8, min_value=None, round_limit=.9):
    min_value = min_value or divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < round_limit * v:         # make sure that round down does not go down by more than 10%
        new_v += divisor
    return new_v


def round_channels(channels, multiplier=1.0, divisor=8, channel_min=None, round_limit=0.9):
    if not multiplier:
        return channels
    return make_divisible(channels * multiplier, divisor, channel_min, round_limit=round_limit)


def _unsupported(what: str):
    raise NotImplementedError(f'torchok_amd MnasNet: {what} not built')


def _decode_block_str(block_str: str) -> dict:
    """[timm] _decode_block_str for the 'ds' / 'ir' block types with the options r k s e c se noskip."""
    ops = block_str.split('_')
    block_type, ops = ops[0], ops[1:]
    if block_type not in ('ds', 'ir'):
        _unsupported(f'block type {block_type!r}')
    opts, noskip = {}, False
    for op in ops:
        if op == 'noskip':
            noskip = True
            continue
        m = re.match(r'^(se|[a-z])(.*)$', op)
        key, value = m.group(1), m.group(2)
        if key not in ('r', 'k', 's', 'e', 'c', 'se'):
            _unsupported(f'block option {op!r}')
        opts[key] = value
    args = dict(block_type=block_type, dw_kernel_size=int(opts['k']), out_chs=int(opts['c']), stride=int(opts['s']),
                se_ratio=float(opts['se']) if 'se' in opts else 0., noskip=noskip)
    if block_type == 'ir':
        args['exp_ratio'] = float(opts.get('e', 1.0))
    return args, int(opts.get('r', 1))


def decode_arch_def(arch_def) -> List[List[dict]]:
    stages = []
    for stack in arch_def:
        blocks = []
        for block_str in stack:
            args, repeats = _decode_block_str(block_str)
            blocks.extend(dict(args) for _ in range(repeats))
        stages.append(blocks)
    return stages


class SqueezeExcite(nn.Module):
    """[timm] efficientnet_blocks.SqueezeExcite (ReLU, sigmoid gate); the two 1x1 convs are parameter containers."""

    def __init__(self, in_chs, rd_ratio=0.25):
        super().__init__()
        rd_channels = round(in_chs * rd_ratio)
        self.conv_reduce = nn.Conv2d(in_chs, rd_channels, 1, bias=True)
        self.conv_expand = nn.Conv2d(rd_channels, in_chs, 1, bias=True)

    def run(self, r, x):
        return EF.squeeze_excite(r, x, self)


class DepthwiseSeparableConv(nn.Module):
    """[timm] 'ds' block: dw conv -> bn + ReLU -> [se] -> 1x1 conv -> bn (-> + x)."""

    def __init__(self, in_chs, out_chs, dw_kernel_size=3, stride=1, noskip=False, se_ratio=0.):
        super().__init__()
        self.has_skip = (stride == 1 and in_chs == out_chs) and not noskip
        self.conv_dw = nn.Conv2d(in_chs, in_chs, dw_kernel_size, stride=stride, padding=dw_kernel_size // 2, groups=in_chs,
                                 bias=False)
        self.bn1 = nn.BatchNorm2d(in_chs)
        self.se = SqueezeExcite(in_chs, rd_ratio=se_ratio) if se_ratio else nn.Identity()
        self.conv_pw = nn.Conv2d(in_chs, out_chs, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(out_chs)

    def forward(self, x):
        r = engine.current_region()
        y = EF.dwconv_bn_act(r, x, self.conv_dw, self.bn1, relu=True)
        if isinstance(self.se, SqueezeExcite):
            y = self.se.run(r, y)
        return EF.conv_bn_act(r, y, self.conv_pw, self.bn2, relu=False, shortcut=x if self.has_skip else None)


class InvertedResidual(nn.Module):
    """[timm] 'ir' block: 1x1 conv -> bn + ReLU -> dw conv -> bn + ReLU -> [se] -> 1x1 conv -> bn (-> + x)."""

    def __init__(self, in_chs, out_chs, dw_kernel_size=3, stride=1, noskip=False, exp_ratio=1.0, se_ratio=0.):
        super().__init__()
        mid_chs = make_divisible(in_chs * exp_ratio)
        self.has_skip = (in_chs == out_chs and stride == 1) and not noskip
        self.conv_pw = nn.Conv2d(in_chs, mid_chs, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid_chs)
        self.conv_dw = nn.Conv2d(mid_chs, mid_chs, dw_kernel_size, stride=stride, padding=dw_kernel_size // 2,
                                 groups=mid_chs, bias=False)
        self.bn2 = nn.BatchNorm2d(mid_chs)
        self.se = SqueezeExcite(mid_chs, rd_ratio=se_ratio) if se_ratio else nn.Identity()
        self.conv_pwl = nn.Conv2d(mid_chs, out_chs, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(out_chs)

    def forward(self, x):
        r = engine.current_region()
        y = EF.conv_bn_act(r, x, self.conv_pw, self.bn1, relu=True)
        y = EF.dwconv_bn_act(r, y, self.conv_dw, self.bn2, relu=True)
        if isinstance(self.se, SqueezeExcite):
            y = self.se.run(r, y)
        return EF.conv_bn_act(r, y, self.conv_pwl, self.bn3, relu=False, shortcut=x if self.has_skip else None)


def _build_blocks(in_chs, block_args, round_chs_fn):
    """[timm] EfficientNetBuilder.__call__ (output stride 32, no drop path): stages of blocks and their feature_info (the last
    block of every stage that is followed by a strided stage, and of the last stage)."""
    stages, features = [], []
    current_stride = 2
    for stack_idx, stack in enumerate(block_args):
        blocks = []
        for block_idx, ba in enumerate(stack):
            ba = dict(ba)
            stride = ba['stride'] if block_idx == 0 else 1
            current_stride *= stride
            out_chs = round_chs_fn(ba['out_chs'])
            bt = ba.pop('block_type')
            se_ratio = ba['se_ratio'] / ba.get('exp_ratio', 1.0)       # se_from_exp=False: the ratio refers to the block input
            if bt == 'ds':
                blocks.append(DepthwiseSeparableConv(in_chs, out_chs, ba['dw_kernel_size'], stride, ba['noskip'], se_ratio))
            else:
                blocks.append(InvertedResidual(in_chs, out_chs, ba['dw_kernel_size'], stride, ba['noskip'], ba['exp_ratio'],
                                               se_ratio))
            in_chs = out_chs
            if block_idx + 1 == len(stack):
                nxt = stack_idx + 1
                if nxt >= len(block_args) or block_args[nxt][0]['stride'] > 1:
                    features.append(dict(stage=stack_idx + 1, reduction=current_stride, num_chs=out_chs,
                                         module=f'blocks.{stack_idx}.{block_idx}'))
        stages.append(nn.Sequential(*blocks))
    return stages, features, in_chs


def _init_weight_goog(m):
    if isinstance(m, nn.Conv2d):
        fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
        m.weight.data.normal_(0, math.sqrt(2.0 / fan_out))
        if m.bias is not None:
            m.bias.data.zero_()
    elif isinstance(m, nn.BatchNorm2d):
        m.weight.data.fill_(1.0)
        m.bias.data.zero_()


class EfficientNet(BaseBackbone):
    """The MnasNet members of the reference's EfficientNet family: stem conv 3x3/s2 + bn + ReLU, the 'ds' / 'ir' stages,
    1x1 head conv + bn + ReLU to `num_features` channels."""

    def __init__(self, block_args, num_features=1280, in_channels=3, stem_size=32, fix_stem=False, output_stride=32,
                 pad_type='', round_chs_fn=round_channels, act_layer=None, norm_layer=None, se_layer=None,
                 drop_path_rate=0.):
        super().__init__(in_channels=in_channels, out_channels=num_features)
        if drop_path_rate > 0:
            _unsupported(f'drop_path_rate={drop_path_rate}')
        if output_stride != 32:
            _unsupported(f'output_stride={output_stride}')
        if act_layer not in (None, nn.ReLU):
            _unsupported(f'act_layer={act_layer}')
        if norm_layer is not None and not (norm_layer is nn.BatchNorm2d or getattr(norm_layer, 'func', None) is nn.BatchNorm2d):
            _unsupported(f'norm_layer={norm_layer}')
        if pad_type not in ('', None) or se_layer is not None:
            _unsupported(f'pad_type={pad_type!r} / se_layer={se_layer}')
        self.num_features = num_features
        if not fix_stem:
            stem_size = round_chs_fn(stem_size)
        self.conv_stem = nn.Conv2d(in_channels, stem_size, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(stem_size)
        stages, self.feature_info, head_chs = _build_blocks(stem_size, block_args, round_chs_fn)
        self.blocks = nn.Sequential(*stages)
        self.conv_head = nn.Conv2d(head_chs, self.num_features, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(self.num_features)
        self.create_hooks()
        self.init_weights()
        self.to(memory_format=torch.channels_last)

    def init_weights(self):
        for m in self.modules():
            _init_weight_goog(m)

    def _run(self, r, x: torch.Tensor, all_features: bool):
        t = r.input(x, c_pad_to=4 if x.shape[1] <= 4 else 8)
        t = EF.conv_bn_act(r, t, self.conv_stem, self.bn1, relu=True)
        wanted = {f['module'] for f in self.feature_info}
        feats = []
        for si, stage in enumerate(self.blocks):
            for bi, block in enumerate(stage):
                t = block(t)
                if all_features and f'blocks.{si}.{bi}' in wanted:
                    feats.append(t)
        if not all_features:
            feats.append(EF.conv_bn_act(r, t, self.conv_head, self.bn2, relu=True))
        return feats

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        with engine.region() as r:
            return r.output(*self._run(r, x, all_features=False))

    def forward_features(self, x: torch.Tensor) -> List[torch.Tensor]:
        with engine.region() as r:
            outs = r.output(*self._run(r, x, all_features=True))
        return [x] + (list(outs) if isinstance(outs, tuple) else [outs])

    def get_stages(self, stage: int) -> nn.Module:
        output = [self.conv_stem, self.bn1]
        layers = list(self.blocks) + [nn.ModuleList([self.conv_head, self.bn2])]
        return nn.ModuleList(output + layers[:stage])


def _create_effnet(variant, pretrained=False, **kwargs):
    for k in ('num_classes', 'global_pool', 'in_chans'):
        kwargs.pop(k, None)
    if pretrained:
        raise RuntimeError(f'{variant}: pretrained weights need a download (no network here); pass '
                           f'pretrained=false and use task.load_checkpoint for local checkpoints')
    for k in ('bn_tf', 'bn_momentum', 'bn_eps'):
        if kwargs.pop(k, None) is not None:
            _unsupported(k)
    return EfficientNet(**kwargs)


def _gen_mnasnet(variant, arch_def, stem_size, channel_multiplier, pretrained, **kwargs):
    def round_chs_fn(c):
        return round_channels(c, multiplier=channel_multiplier)
    return _create_effnet(variant, pretrained, block_args=decode_arch_def(arch_def), stem_size=stem_size,
                          round_chs_fn=round_chs_fn, **kwargs)


_MNASNET_A1 = [['ds_r1_k3_s1_e1_c16_noskip'], ['ir_r2_k3_s2_e6_c24'], ['ir_r3_k5_s2_e3_c40_se0.25'], ['ir_r4_k3_s2_e6_c80'],
               ['ir_r2_k3_s1_e6_c112_se0.25'], ['ir_r3_k5_s2_e6_c160_se0.25'], ['ir_r1_k3_s1_e6_c320']]
_MNASNET_B1 = [['ds_r1_k3_s1_c16_noskip'], ['ir_r3_k3_s2_e3_c24'], ['ir_r3_k5_s2_e3_c40'], ['ir_r3_k5_s2_e6_c80'],
               ['ir_r2_k3_s1_e6_c96'], ['ir_r4_k5_s2_e6_c192'], ['ir_r1_k3_s1_e6_c320_noskip']]
_MNASNET_SMALL = [['ds_r1_k3_s1_c8'], ['ir_r1_k3_s2_e3_c16'], ['ir_r2_k3_s2_e6_c16'], ['ir_r4_k5_s2_e6_c32_se0.25'],
                  ['ir_r3_k3_s1_e6_c32_se0.25'], ['ir_r3_k5_s2_e6_c88_se0.25'], ['ir_r1_k3_s1_e6_c144']]


def _entry(name, arch_def, stem_size, multiplier, doc):
    def entry(pretrained=False, **kwargs):
        return _gen_mnasnet(name, arch_def, stem_size, multiplier, pretrained, **kwargs)
    entry.__name__ = entry.__qualname__ = name
    entry.__doc__ = doc
    return BACKBONES.register_class(entry)


mnasnet_050 = _entry('mnasnet_050', _MNASNET_B1, 32, 0.5, 'MNASNet B1, depth multiplier of 0.5 (efficientnet.py:1181-1185)')
mnasnet_075 = _entry('mnasnet_075', _MNASNET_B1, 32, 0.75, 'MNASNet B1, depth multiplier of 0.75')
mnasnet_100 = _entry('mnasnet_100', _MNASNET_B1, 32, 1.0, 'MNASNet B1, depth multiplier of 1.0')
mnasnet_b1 = _entry('mnasnet_b1', _MNASNET_B1, 32, 1.0, 'MNASNet B1, depth multiplier of 1.0 (= mnasnet_100)')
mnasnet_140 = _entry('mnasnet_140', _MNASNET_B1, 32, 1.4, 'MNASNet B1, depth multiplier of 1.4')
semnasnet_050 = _entry('semnasnet_050', _MNASNET_A1, 32, 0.5, 'MNASNet A1 (w/ SE), depth multiplier of 0.5')
semnasnet_075 = _entry('semnasnet_075', _MNASNET_A1, 32, 0.75, 'MNASNet A1 (w/ SE), depth multiplier of 0.75')
semnasnet_100 = _entry('semnasnet_100', _MNASNET_A1, 32, 1.0, 'MNASNet A1 (w/ SE), depth multiplier of 1.0')
mnasnet_a1 = _entry('mnasnet_a1', _MNASNET_A1, 32, 1.0, 'MNASNet A1 (w/ SE), depth multiplier of 1.0 (= semnasnet_100)')
semnasnet_140 = _entry('semnasnet_140', _MNASNET_A1, 32, 1.4, 'MNASNet A1 (w/ SE), depth multiplier of 1.4')
mnasnet_small = _entry('mnasnet_small', _MNASNET_SMALL, 8, 1.0, 'MNASNet Small, depth multiplier of 1.0')
