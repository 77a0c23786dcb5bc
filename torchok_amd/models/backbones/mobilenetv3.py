"""MobileNetV3 backbones on the MI355X engine.

Mirrors the reference wiring ``torchok/models/backbones/mobilenetv3.py``: ``MobileNetV3`` (:108-170), ``_gen_mobilenet_v3``
(:217-311) and the seven large / small entry points (:413-463), with the [timm 0.6.13] ``decode_arch_def``,
``EfficientNetBuilder`` (``se_from_exp=True``), ``DepthwiseSeparableConv``, ``InvertedResidual``, ``ConvBnAct`` and
``SqueezeExcite(gate_layer='hard_sigmoid', force_act_layer=nn.ReLU, rd_round_fn=round_channels)`` semantics restated here.
Module / parameter names are those of timm, so reference checkpoints load.

The blocks, the block-string decoder and the builder are those of ``_efficientnet_blocks.py``, shared with
``efficientnet.py``; this family passes what differs: the 'cn' block type and the 'nre' option (a block marked ``nre`` runs its
units with ReLU, every other block with the model's activation, hard-swish: ``act='hard_swish'``, the mask-less path of
csrc/bn.hip), the squeeze-excite that keeps its ReLU inside, gates with a hard sigmoid and rounds its width with
``round_channels``, ``se_from_exp=True`` and the stem feature.  Not built: ``mobilenetv3_rw``, the ``tf_*`` variants (asymmetric
"same" padding), the ``minimal`` variants, ``fbnetv3_*`` and ``lcnet_*``.
"""
from functools import partial
from typing import List

import torch
import torch.nn as nn

from ... import engine
from ...constructor import BACKBONES
from ...engine import functional as EF
from ..base import BaseBackbone
from . import _efficientnet_blocks as B
from ._efficientnet_blocks import init_weight_goog, round_channels


def _unsupported(what: str):
    raise NotImplementedError(f'torchok_amd MobileNetV3: {what} not built')


# the family's arguments to the shared blocks: hard-swish where a block is not marked 'nre', the hard-sigmoid squeeze-excite
# with the reduced width rounded by round_channels (a multiple of 8)
SqueezeExcite = partial(B.SqueezeExcite, rd_round_fn=round_channels, gate='hard_sigmoid')
DepthwiseSeparableConv = partial(B.DepthwiseSeparableConv, act=EF.HARD_SWISH, se_layer=SqueezeExcite)
InvertedResidual = partial(B.InvertedResidual, act=EF.HARD_SWISH, se_layer=SqueezeExcite)
ConvBnAct = partial(B.ConvBnAct, act=EF.HARD_SWISH)


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
        stages, feature_info, out_chs = B.build_blocks(stem_size, block_args, round_chs_fn, se_from_exp=True, stem_feature=True,
                                                       act=EF.HARD_SWISH, se_layer=SqueezeExcite)
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
            init_weight_goog(m)

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
    return MobileNetV3(block_args=B.decode_arch_def(_SMALL if small else _LARGE, _unsupported, ('ds', 'ir', 'cn'), nre=True),
                       num_features=1024 if small else 1280,
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
