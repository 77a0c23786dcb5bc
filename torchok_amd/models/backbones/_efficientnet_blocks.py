"""The block family of the reference's ``efficientnet.py`` and ``mobilenetv3.py`` ([timm 0.6.13] efficientnet_builder /
efficientnet_blocks, restated): the block-string decoder, ``SqueezeExcite``, the 'ds' / 'ir' / 'cn' blocks and the builder.

Each ``conv -> bn -> act`` group is one engine unit: 1x1 and dense convolutions on ``conv_bn_act`` (the projection of a block
with a skip connection adds the block input before nothing else: ``relu=False, shortcut=x``), the depthwise convolution on
``dwconv_bn_act``, the squeeze-excite on ``squeeze_excite``.  What differs between the families comes in as arguments: the
block types and options the decoder accepts, the activation of a block that is not marked 'nre' (`act`), the squeeze-excite
module (`se_layer`: width rule and gate), `se_from_exp` and the stem feature.  Module and parameter names, and the order in
which a block assigns its submodules, are timm's: state_dict keys, `modules()` order and seeded initial weights depend on it.
"""
import math
import re
from typing import List

import torch.nn as nn

from ... import engine
from ...engine import functional as EF


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


def decode_block_str(block_str: str, unsupported, block_types=('ds', 'ir'), nre=False):
    """[timm] _decode_block_str for `block_types` with the options r k s e c se noskip (and nre where the family has it);
    everything else goes to the family's `unsupported`."""
    ops = block_str.split('_')
    block_type, ops = ops[0], ops[1:]
    if block_type not in block_types:
        unsupported(f'block type {block_type!r}')
    opts, noskip, relu = {}, False, False
    for op in ops:
        if op == 'noskip':
            noskip = True
            continue
        if op == 'nre' and nre:
            relu = True
            continue
        m = re.match(r'^(se|[a-z])(.*)$', op)
        key, value = m.group(1), m.group(2)
        if key not in ('r', 'k', 's', 'e', 'c', 'se'):
            unsupported(f'block option {op!r}')
        opts[key] = value
    args = dict(block_type=block_type, kernel_size=int(opts['k']), out_chs=int(opts['c']), stride=int(opts['s']), relu=relu)
    if block_type != 'cn':
        args.update(se_ratio=float(opts['se']) if 'se' in opts else 0., noskip=noskip)
    if block_type == 'ir':
        args['exp_ratio'] = float(opts.get('e', 1.0))
    return args, int(opts.get('r', 1))


def scale_stage_depth(repeats: List[int], depth_multiplier=1.0, depth_trunc='ceil') -> List[int]:
    """[timm] _scale_stage_depth: the repeats of one stage's block definitions under a depth multiplier.  The scaled total of
    the stage is ceil (or round) of sum(repeats) * multiplier; it is handed out from the last definition to the first, each
    taking its share of what is left (at least 1), so the first definition is the least likely to grow."""
    num_repeat = sum(repeats)
    if depth_trunc == 'round':
        num_repeat_scaled = max(1, round(num_repeat * depth_multiplier))
    else:
        num_repeat_scaled = int(math.ceil(num_repeat * depth_multiplier))
    scaled = []
    for r in reversed(repeats):
        rs = max(1, round(r / num_repeat * num_repeat_scaled))
        scaled.append(rs)
        num_repeat -= r
        num_repeat_scaled -= rs
    return scaled[::-1]


def decode_arch_def(arch_def, unsupported, block_types=('ds', 'ir'), nre=False, depth_multiplier=1.0, depth_trunc='ceil',
                    fix_first_last=False) -> List[List[dict]]:
    """[timm] decode_arch_def.  `depth_multiplier` scales every stage's repeats (scale_stage_depth), except the first and the
    last stage under `fix_first_last`; at the default 1.0 a stage keeps the repeats its strings name."""
    if depth_trunc not in ('ceil', 'round'):
        unsupported(f'depth_trunc={depth_trunc!r}')
    stages = []
    for stack_idx, stack in enumerate(arch_def):
        decoded = [decode_block_str(block_str, unsupported, block_types, nre) for block_str in stack]
        repeats = [r for _, r in decoded]
        if depth_multiplier != 1.0 and not (fix_first_last and stack_idx in (0, len(arch_def) - 1)):
            repeats = scale_stage_depth(repeats, depth_multiplier, depth_trunc)
        blocks = []
        for (args, _), rep in zip(decoded, repeats):
            blocks.extend(dict(args) for _ in range(rep))
        stages.append(blocks)
    return stages


class SqueezeExcite(nn.Module):
    """[timm] efficientnet_blocks.SqueezeExcite with ReLU inside; the two 1x1 convs are parameter containers.  MnasNet: the
    sigmoid gate and round() for the reduced width; MobileNetV3: 'hard_sigmoid' and round_channels (a multiple of 8)."""

    def __init__(self, in_chs, rd_ratio=0.25, rd_round_fn=round, gate='sigmoid'):
        super().__init__()
        rd_channels = rd_round_fn(in_chs * rd_ratio)
        self.gate = gate
        self.conv_reduce = nn.Conv2d(in_chs, rd_channels, 1, bias=True)
        self.conv_expand = nn.Conv2d(rd_channels, in_chs, 1, bias=True)

    def run(self, r, x):
        return EF.squeeze_excite(r, x, self, gate=self.gate)


def _act_kw(relu: bool, act):
    """(relu=, act=) of a unit that activates: ReLU for an 'nre' block and for a family without `act`, else the family's."""
    return dict(relu=True) if relu or act is None else dict(relu=False, act=act)


class DepthwiseSeparableConv(nn.Module):
    """[timm] 'ds' block: dw conv -> bn + act -> [se] -> 1x1 conv -> bn (-> + x)."""

    def __init__(self, in_chs, out_chs, dw_kernel_size=3, stride=1, noskip=False, se_ratio=0., relu=False, act=None,
                 se_layer=SqueezeExcite):
        super().__init__()
        self.has_skip = (stride == 1 and in_chs == out_chs) and not noskip
        self.relu = relu or act is None
        self.act_kw = _act_kw(relu, act)
        self.conv_dw = nn.Conv2d(in_chs, in_chs, dw_kernel_size, stride=stride, padding=dw_kernel_size // 2, groups=in_chs,
                                 bias=False)
        self.bn1 = nn.BatchNorm2d(in_chs)
        self.se = se_layer(in_chs, rd_ratio=se_ratio) if se_ratio else nn.Identity()
        self.conv_pw = nn.Conv2d(in_chs, out_chs, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(out_chs)

    def forward(self, x):
        r = engine.current_region()
        y = EF.dwconv_bn_act(r, x, self.conv_dw, self.bn1, **self.act_kw)
        if isinstance(self.se, SqueezeExcite):
            y = self.se.run(r, y)
        return EF.conv_bn_act(r, y, self.conv_pw, self.bn2, relu=False, shortcut=x if self.has_skip else None)


class InvertedResidual(nn.Module):
    """[timm] 'ir' block: 1x1 conv -> bn + act -> dw conv -> bn + act -> [se] -> 1x1 conv -> bn (-> + x)."""

    def __init__(self, in_chs, out_chs, dw_kernel_size=3, stride=1, noskip=False, exp_ratio=1.0, se_ratio=0., relu=False,
                 act=None, se_layer=SqueezeExcite):
        super().__init__()
        mid_chs = make_divisible(in_chs * exp_ratio)
        self.has_skip = (in_chs == out_chs and stride == 1) and not noskip
        self.relu = relu or act is None
        self.act_kw = _act_kw(relu, act)
        self.conv_pw = nn.Conv2d(in_chs, mid_chs, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid_chs)
        self.conv_dw = nn.Conv2d(mid_chs, mid_chs, dw_kernel_size, stride=stride, padding=dw_kernel_size // 2,
                                 groups=mid_chs, bias=False)
        self.bn2 = nn.BatchNorm2d(mid_chs)
        self.se = se_layer(mid_chs, rd_ratio=se_ratio) if se_ratio else nn.Identity()
        self.conv_pwl = nn.Conv2d(mid_chs, out_chs, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(out_chs)

    def forward(self, x):
        r = engine.current_region()
        y = EF.conv_bn_act(r, x, self.conv_pw, self.bn1, **self.act_kw)
        y = EF.dwconv_bn_act(r, y, self.conv_dw, self.bn2, **self.act_kw)
        if isinstance(self.se, SqueezeExcite):
            y = self.se.run(r, y)
        return EF.conv_bn_act(r, y, self.conv_pwl, self.bn3, relu=False, shortcut=x if self.has_skip else None)


class ConvBnAct(nn.Module):
    """[timm] 'cn' block: conv -> bn + act (no skip: the block strings built here never ask for one)."""

    def __init__(self, in_chs, out_chs, kernel_size=1, stride=1, relu=False, act=None):
        super().__init__()
        self.has_skip = False
        self.relu = relu or act is None
        self.act_kw = _act_kw(relu, act)
        self.conv = nn.Conv2d(in_chs, out_chs, kernel_size, stride=stride, padding=kernel_size // 2, bias=False)
        self.bn1 = nn.BatchNorm2d(out_chs)

    def forward(self, x):
        return EF.conv_bn_act(engine.current_region(), x, self.conv, self.bn1, **self.act_kw)


def build_blocks(in_chs, block_args, round_chs_fn, se_from_exp=False, stem_feature=False, act=None, se_layer=SqueezeExcite):
    """[timm] EfficientNetBuilder.__call__ (output stride 32, no drop path): stages of blocks and their feature_info — the
    stem (`stem_feature`, when the first block is strided), then the last block of every stage that is followed by a strided
    stage, and of the last stage.  se_from_exp=False: a block's squeeze-excite ratio refers to the block input, not to the
    expanded width."""
    stages, features = [], []
    current_stride = 2
    if stem_feature and block_args[0][0]['stride'] > 1:
        features.append(dict(stage=0, reduction=current_stride, num_chs=in_chs, module='act1'))
    for stack_idx, stack in enumerate(block_args):
        blocks = []
        for block_idx, ba in enumerate(stack):
            stride = ba['stride'] if block_idx == 0 else 1
            current_stride *= stride
            out_chs = round_chs_fn(ba['out_chs'])
            bt = ba['block_type']
            if bt == 'cn':
                blocks.append(ConvBnAct(in_chs, out_chs, ba['kernel_size'], stride, ba['relu'], act))
            else:
                se_ratio = ba['se_ratio'] if se_from_exp else ba['se_ratio'] / ba.get('exp_ratio', 1.0)
                if bt == 'ds':
                    blocks.append(DepthwiseSeparableConv(in_chs, out_chs, ba['kernel_size'], stride, ba['noskip'], se_ratio,
                                                         ba['relu'], act, se_layer))
                else:
                    blocks.append(InvertedResidual(in_chs, out_chs, ba['kernel_size'], stride, ba['noskip'], ba['exp_ratio'],
                                                   se_ratio, ba['relu'], act, se_layer))
            in_chs = out_chs
            if block_idx + 1 == len(stack):
                nxt = stack_idx + 1
                if nxt >= len(block_args) or block_args[nxt][0]['stride'] > 1:
                    features.append(dict(stage=stack_idx + 1, reduction=current_stride, num_chs=out_chs,
                                         module=f'blocks.{stack_idx}.{block_idx}'))
        stages.append(nn.Sequential(*blocks))
    return stages, features, in_chs


def init_weight_goog(m):
    if isinstance(m, nn.Conv2d):
        fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
        m.weight.data.normal_(0, math.sqrt(2.0 / fan_out))
        if m.bias is not None:
            m.bias.data.zero_()
    elif isinstance(m, nn.BatchNorm2d):
        m.weight.data.fill_(1.0)
        m.bias.data.zero_()
