"""MobileNetV3 backbones on the MI355X engine.

Mirrors the reference wiring ``torchok/models/backbones/mobilenetv3.py``: ``MobileNetV3`` (:108-170), ``_gen_mobilenet_v3``
(:217-311) and the seven large / small entry points (:413-463), with the [timm 0.6.13] ``decode_arch_def``,
``EfficientNetBuilder`` (``se_from_exp=True``), ``DepthwiseSeparableConv``, ``InvertedResidual``, ``ConvBnAct`` and
``SqueezeExcite(gate_layer='hard_sigmoid', force_act_layer=nn.ReLU, rd_round_fn=round_channels)`` semantics restated here.
Module / parameter names are those of timm, so reference checkpoints load.

Each ``conv -> bn -> act`` group is one engine unit, as in ``efficientnet.py``; a block marked ``nre`` runs them with ReLU,
every other block with the model's activation, hard-swish (``act='hard_swish'``: the mask-less path of csrc/act.hip).  The
squeeze-excite keeps its ReLU inside and gates with a hard sigmoid.  The decoder and the builder live here, beside those of
``efficientnet.py``, so that what the MnasNet entry points accept and refuse does not move; ``make_divisible``,
``round_channels`` and ``_init_weight_goog`` are shared.  Not built: ``mobilenetv3_rw``, the ``tf_*`` variants (asymmetric
"same" padding), the ``minimal`` variants, ``fbnetv3_*`` and ``lcnet_*``.
"""
import re
from typing import List

import torch
import torch.nn as nn

from ... import engine
from ...constructor import BACKBONES
from ...engine import functional as EF
from ..base import BaseBackbone
from .efficientnet import _init_weight_goog, make_divisible, round_channels


def _unsupported(what: str):
    raise NotImplementedError(f'torchok_amd MobileNetV3: {what} not built')


def _decode_block_str(block_str: str):
    """[timm] _decode_block_str for the 'ds' / 'ir' / 'cn' block types with the options r k s e c se nre noskip."""
    ops = block_str.split('_')
    block_type, ops = ops[0], ops[1:]
    if block_type not in ('ds', 'ir', 'cn'):
        _unsupported(f'block type {block_type!r}')
    opts, noskip, relu = {}, False, False
    for op in ops:
        if op == 'noskip':
            noskip = True
            continue
        if op == 'nre':
            relu = True
            continue
        m = re.match(r'^(se|[a-z])(.*)$', op)
        key, value = m.group(1), m.group(2)
        if key not in ('r', 'k', 's', 'e', 'c', 'se'):
            _unsupported(f'block option {op!r}')
        opts[key] = value
    args = dict(block_type=block_type, kernel_size=int(opts['k']), out_chs=int(opts['c']), stride=int(opts['s']), relu=relu)
    if block_type != 'cn':
        args.update(se_ratio=float(opts['se']) if 'se' in opts else 0., noskip=noskip)
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
    """[timm] efficientnet_blocks.SqueezeExcite with ReLU inside, the hard-sigmoid gate and the reduced width rounded by
    round_channels (a multiple of 8); the two 1x1 convs are parameter containers."""

    def __init__(self, in_chs, rd_ratio=0.25):
        super().__init__()
        rd_channels = round_channels(in_chs * rd_ratio)
        self.conv_reduce = nn.Conv2d(in_chs, rd_channels, 1, bias=True)
        self.conv_expand = nn.Conv2d(rd_channels, in_chs, 1, bias=True)

    def run(self, r, x):
        return EF.squeeze_excite(r, x, self, gate='hard_sigmoid')


def _act(relu: bool):
    """(relu, act) of a unit that activates: ReLU for an 'nre' block, the model's hard-swish otherwise."""
    return dict(relu=True) if relu else dict(relu=False, act=EF.HARD_SWISH)


class DepthwiseSeparableConv(nn.Module):
    """[timm] 'ds' block: dw conv -> bn + act -> [se] -> 1x1 conv -> bn (-> + x)."""

    def __init__(self, in_chs, out_chs, dw_kernel_size=3, stride=1, noskip=False, se_ratio=0., relu=False):
        super().__init__()
        self.has_skip = (stride == 1 and in_chs == out_chs) and not noskip
        self.relu = relu
        self.conv_dw = nn.Conv2d(in_chs, in_chs, dw_kernel_size, stride=stride, padding=dw_kernel_size // 2, groups=in_chs,
                                 bias=False)
        self.bn1 = nn.BatchNorm2d(in_chs)
        self.se = SqueezeExcite(in_chs, rd_ratio=se_ratio) if se_ratio else nn.Identity()
        self.conv_pw = nn.Conv2d(in_chs, out_chs, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(out_chs)

    def forward(self, x):
        r = engine.current_region()
        y = EF.dwconv_bn_act(r, x, self.conv_dw, self.bn1, **_act(self.relu))
        if isinstance(self.se, SqueezeExcite):
            y = self.se.run(r, y)
        return EF.conv_bn_act(r, y, self.conv_pw, self.bn2, relu=False, shortcut=x if self.has_skip else None)


class InvertedResidual(nn.Module):
    """[timm] 'ir' block: 1x1 conv -> bn + act -> dw conv -> bn + act -> [se] -> 1x1 conv -> bn (-> + x).  The
    squeeze-excite ratio refers to the expanded width (se_from_exp=True)."""

    def __init__(self, in_chs, out_chs, dw_kernel_size=3, stride=1, noskip=False, exp_ratio=1.0, se_ratio=0., relu=False):
        super().__init__()
        mid_chs = make_divisible(in_chs * exp_ratio)
        self.has_skip = (in_chs == out_chs and stride == 1) and not noskip
        self.relu = relu
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
        y = EF.conv_bn_act(r, x, self.conv_pw, self.bn1, **_act(self.relu))
        y = EF.dwconv_bn_act(r, y, self.conv_dw, self.bn2, **_act(self.relu))
        if isinstance(self.se, SqueezeExcite):
            y = self.se.run(r, y)
        return EF.conv_bn_act(r, y, self.conv_pwl, self.bn3, relu=False, shortcut=x if self.has_skip else None)


class ConvBnAct(nn.Module):
    """[timm] 'cn' block: conv -> bn + act (no skip: the block strings of this family never ask for one)."""

    def __init__(self, in_chs, out_chs, kernel_size=1, stride=1, relu=False):
        super().__init__()
        self.has_skip = False
        self.relu = relu
        self.conv = nn.Conv2d(in_chs, out_chs, kernel_size, stride=stride, padding=kernel_size // 2, bias=False)
        self.bn1 = nn.BatchNorm2d(out_chs)

    def forward(self, x):
        return EF.conv_bn_act(engine.current_region(), x, self.conv, self.bn1, **_act(self.relu))


def _build_blocks(in_chs, block_args, round_chs_fn):
    """[timm] EfficientNetBuilder.__call__ (output stride 32, no drop path, se_from_exp=True): stages of blocks and their
    feature_info — the stem when the first block is strided, then the last block of every stage that is followed by a strided
    stage, and of the last stage."""
    stages, features = [], []
    current_stride = 2
    if block_args[0][0]['stride'] > 1:
        features.append(dict(stage=0, reduction=current_stride, num_chs=in_chs, module='act1'))
    for stack_idx, stack in enumerate(block_args):
        blocks = []
        for block_idx, ba in enumerate(stack):
            stride = ba['stride'] if block_idx == 0 else 1
            current_stride *= stride
            out_chs = round_chs_fn(ba['out_chs'])
            bt = ba['block_type']
            if bt == 'ds':
                blocks.append(DepthwiseSeparableConv(in_chs, out_chs, ba['kernel_size'], stride, ba['noskip'], ba['se_ratio'],
                                                     ba['relu']))
            elif bt == 'ir':
                blocks.append(InvertedResidual(in_chs, out_chs, ba['kernel_size'], stride, ba['noskip'], ba['exp_ratio'],
                                               ba['se_ratio'], ba['relu']))
            else:
                blocks.append(ConvBnAct(in_chs, out_chs, ba['kernel_size'], stride, ba['relu']))
            in_chs = out_chs
            if block_idx + 1 == len(stack):
                nxt = stack_idx + 1
                if nxt >= len(block_args) or block_args[nxt][0]['stride'] > 1:
                    features.append(dict(stage=stack_idx + 1, reduction=current_stride, num_chs=out_chs,
                                         module=f'blocks.{stack_idx}.{block_idx}'))
        stages.append(nn.Sequential(*blocks))
    return stages, features, in_chs


class MobileNetV3(BaseBackbone):
    """The large / small members of the reference's MobileNetV3 family: stem conv 3x3/s2 + bn + hard-swish, then the 'ds' /
    'ir' stages and the closing 1x1 'cn' block.  The backbone ends at `blocks` (no conv_head).

    One deliberate deviation: the reference passes ``out_channels=num_features`` (1280 / 1024, the width of the classifier's
    conv_head it does not build) although the map it returns has 960 / 576 channels times the multiplier, so a pooling + head
    chained on ``backbone.out_channels``, as the Tasks do, cannot run there.  Here ``out_channels`` is the real width of the
    returned map; ``num_features`` keeps the reference's value as an attribute."""

    def __init__(self, block_args, in_channels=3, stem_size=16, fix_stem=False, num_features=1280, pad_type='',
                 act_layer=None, norm_layer=None, se_layer=None, se_from_exp=True, round_chs_fn=round_channels,
                 output_stride=32, drop_path_rate=0.):
        if drop_path_rate > 0:
            _unsupported(f'drop_path_rate={drop_path_rate}')
        if output_stride != 32:
            _unsupported(f'output_stride={output_stride}')
        if act_layer not in (None, nn.Hardswish):
            _unsupported(f'act_layer={act_layer}')
        if norm_layer is not None and not (norm_layer is nn.BatchNorm2d or getattr(norm_layer, 'func', None) is nn.BatchNorm2d):
            _unsupported(f'norm_layer={norm_layer}')
        if pad_type not in ('', None) or se_layer is not None or not se_from_exp:
            _unsupported(f'pad_type={pad_type!r} / se_layer={se_layer} / se_from_exp={se_from_exp}')
        if not fix_stem:
            stem_size = round_chs_fn(stem_size)
        conv_stem = nn.Conv2d(in_channels, stem_size, 3, stride=2, padding=1, bias=False)
        bn1 = nn.BatchNorm2d(stem_size)
        stages, feature_info, out_chs = _build_blocks(stem_size, block_args, round_chs_fn)
        super().__init__(in_channels=in_channels, out_channels=out_chs)
        self.num_features = num_features
        self.conv_stem, self.bn1 = conv_stem, bn1
        self.act1 = nn.Hardswish()          # no parameters: the activation runs inside the stem unit
        self.blocks = nn.Sequential(*stages)
        self.feature_info = feature_info
        self.create_hooks()
        self.init_weights()
        self.to(memory_format=torch.channels_last)

    def init_weights(self):
        for m in self.modules():
            _init_weight_goog(m)

    def _run(self, r, x: torch.Tensor, all_features: bool):
        t = r.input(x, c_pad_to=4 if x.shape[1] <= 4 else 8)
        t = EF.conv_bn_act(r, t, self.conv_stem, self.bn1, act=EF.HARD_SWISH)
        wanted = {f['module'] for f in self.feature_info}
        feats = [t] if all_features and 'act1' in wanted else []
        for si, stage in enumerate(self.blocks):
            for bi, block in enumerate(stage):
                t = block(t)
                if all_features and f'blocks.{si}.{bi}' in wanted:
                    feats.append(t)
        return feats if all_features else [t]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        with engine.region() as r:
            return r.output(*self._run(r, x, all_features=False))

    def forward_features(self, x: torch.Tensor) -> List[torch.Tensor]:
        with engine.region() as r:
            outs = r.output(*self._run(r, x, all_features=True))
        return [x] + (list(outs) if isinstance(outs, tuple) else [outs])

    def get_stages(self, stage: int) -> nn.Module:
        return nn.ModuleList([self.conv_stem, self.bn1, self.act1] + list(self.blocks[:stage]))


_LARGE = [['ds_r1_k3_s1_e1_c16_nre'], ['ir_r1_k3_s2_e4_c24_nre', 'ir_r1_k3_s1_e3_c24_nre'], ['ir_r3_k5_s2_e3_c40_se0.25_nre'],
          ['ir_r1_k3_s2_e6_c80', 'ir_r1_k3_s1_e2.5_c80', 'ir_r2_k3_s1_e2.3_c80'], ['ir_r2_k3_s1_e6_c112_se0.25'],
          ['ir_r3_k5_s2_e6_c160_se0.25'], ['cn_r1_k1_s1_c960']]
_SMALL = [['ds_r1_k3_s2_e1_c16_se0.25_nre'], ['ir_r1_k3_s2_e4.5_c24_nre', 'ir_r1_k3_s1_e3.67_c24_nre'],
          ['ir_r1_k5_s2_e4_c40_se0.25', 'ir_r2_k5_s1_e6_c40_se0.25'], ['ir_r2_k5_s1_e3_c48_se0.25'],
          ['ir_r3_k5_s2_e6_c96_se0.25'], ['cn_r1_k1_s1_c576']]


def _gen_mobilenet_v3(variant, channel_multiplier=1.0, pretrained=False, **kwargs):
    for k in ('num_classes', 'global_pool', 'in_chans', 'head_bias'):
        kwargs.pop(k, None)
    if pretrained:
        raise RuntimeError(f'{variant}: pretrained weights need a download (no network here); pass '
                           f'pretrained=false and use task.load_checkpoint for local checkpoints')
    for k in ('bn_tf', 'bn_momentum', 'bn_eps'):
        if kwargs.pop(k, None) is not None:
            _unsupported(k)
    small = 'small' in variant

    def round_chs_fn(c):
        return round_channels(c, multiplier=channel_multiplier)
    return MobileNetV3(block_args=decode_arch_def(_SMALL if small else _LARGE), num_features=1024 if small else 1280,
                       stem_size=16, fix_stem=channel_multiplier < 0.75, round_chs_fn=round_chs_fn, **kwargs)


def _entry(name, multiplier, doc):
    def entry(pretrained=False, **kwargs):
        return _gen_mobilenet_v3(name, multiplier, pretrained=pretrained, **kwargs)
    entry.__name__ = entry.__qualname__ = name
    entry.__doc__ = doc
    return BACKBONES.register_class(entry)


mobilenetv3_large_075 = _entry('mobilenetv3_large_075', 0.75, 'MobileNet V3 large, channel multiplier 0.75 (mobilenetv3.py:413-417)')
mobilenetv3_large_100 = _entry('mobilenetv3_large_100', 1.0, 'MobileNet V3 large')
mobilenetv3_large_100_miil = _entry('mobilenetv3_large_100_miil', 1.0, 'MobileNet V3 large (the MIIL ImageNet-1k checkpoint)')
mobilenetv3_large_100_miil_in21k = _entry('mobilenetv3_large_100_miil_in21k', 1.0,
                                          'MobileNet V3 large (the MIIL ImageNet-21k checkpoint)')
mobilenetv3_small_050 = _entry('mobilenetv3_small_050', 0.5, 'MobileNet V3 small, channel multiplier 0.5 (fixed 16-channel stem)')
mobilenetv3_small_075 = _entry('mobilenetv3_small_075', 0.75, 'MobileNet V3 small, channel multiplier 0.75')
mobilenetv3_small_100 = _entry('mobilenetv3_small_100', 1.0, 'MobileNet V3 small')
