"""MnasNet and EfficientNet-Lite backbones on the MI355X engine.

Mirrors the reference wiring ``torchok/models/backbones/efficientnet.py``: ``EfficientNet`` (:506-575), ``_gen_mnasnet_a1`` /
``_b1`` / ``_small`` (:583-681) and the MnasNet entry points (:1181-1254), ``_gen_efficientnet_lite`` (:890-928) and the five
EfficientNet-Lite entry points (:1528-1569), with the [timm 0.6.13] ``decode_arch_def``,
``EfficientNetBuilder``, ``DepthwiseSeparableConv``, ``InvertedResidual``, ``SqueezeExcite``, ``round_channels`` and
``_init_weight_goog`` semantics restated in ``_efficientnet_blocks.py``.  Module / parameter names are those of timm, so reference checkpoints load.

The blocks, the block-string decoder and the builder are those of ``_efficientnet_blocks.py``, shared with ``mobilenetv3.py``;
MnasNet takes them with their defaults: ReLU, the 'ds' / 'ir' block types without the 'nre' option, the sigmoid
squeeze-excite on the block input's width (``se_from_exp=False``), no stem feature.  EfficientNet-Lite has no squeeze-excite
and runs the stem, every block and the head with ReLU6 (``act='relu6'``, the mask-less path of csrc/bn.hip); its stage depths
follow the decoder's depth multiplier with the first and the last stage fixed.  The SiLU families and the other ReLU6 ones
(EfficientNet B*, MobileNetV2, FBNet, the ``tf_*`` Lite variants with their asymmetric "same" padding) stay unregistered.
"""
from typing import List

import torch
import torch.nn as nn

from ... import engine
from ...constructor import BACKBONES
from ...engine import functional as EF
from ..base import BaseBackbone
from ._efficientnet_blocks import DepthwiseSeparableConv, InvertedResidual, SqueezeExcite  # noqa: F401  (the family's blocks)
from ._efficientnet_blocks import _act_kw, build_blocks, decode_arch_def, init_weight_goog, round_channels


def _unsupported(what: str):
    raise NotImplementedError(f'torchok_amd MnasNet / EfficientNet-Lite: {what} not built')


_ACT_LAYERS = {None: None, nn.ReLU: None, 'relu': None, nn.ReLU6: EF.RELU6, 'relu6': EF.RELU6}


def _resolve_act_layer(act_layer):
    """The blocks' `act` of an `act_layer`: None (ReLU) or EF.RELU6; nothing else is built."""
    try:
        return _ACT_LAYERS[act_layer]
    except (KeyError, TypeError):
        _unsupported(f'act_layer={act_layer}')


class EfficientNet(BaseBackbone):
    """The MnasNet and EfficientNet-Lite members of the reference's EfficientNet family: stem conv 3x3/s2 + bn + act, the
    'ds' / 'ir' stages, 1x1 head conv + bn + act to `num_features` channels; act is ReLU or ReLU6 (`act_layer`), one for the
    stem, the blocks and the head."""

    def __init__(self, block_args, num_features=1280, in_channels=3, stem_size=32, fix_stem=False, output_stride=32,
                 pad_type='', round_chs_fn=round_channels, act_layer=None, norm_layer=None, se_layer=None,
                 drop_path_rate=0.):
        super().__init__(in_channels=in_channels, out_channels=num_features)
        if drop_path_rate > 0:
            _unsupported(f'drop_path_rate={drop_path_rate}')
        if output_stride != 32:
            _unsupported(f'output_stride={output_stride}')
        self.act = _resolve_act_layer(act_layer)
        if norm_layer is not None and not (norm_layer is nn.BatchNorm2d or getattr(norm_layer, 'func', None) is nn.BatchNorm2d):
            _unsupported(f'norm_layer={norm_layer}')
        if pad_type not in ('', None) or se_layer is not None:
            _unsupported(f'pad_type={pad_type!r} / se_layer={se_layer}')
        self.num_features = num_features
        if not fix_stem:
            stem_size = round_chs_fn(stem_size)
        self.conv_stem = nn.Conv2d(in_channels, stem_size, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(stem_size)
        stages, self.feature_info, head_chs = build_blocks(stem_size, block_args, round_chs_fn, act=self.act)
        self.blocks = nn.Sequential(*stages)
        self.conv_head = nn.Conv2d(head_chs, self.num_features, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(self.num_features)
        self.create_hooks()
        self.init_weights()
        self.to(memory_format=torch.channels_last)

    def init_weights(self):
        for m in self.modules():
            init_weight_goog(m)

    def _run(self, r, x: torch.Tensor, all_features: bool):
        t = r.input(x, c_pad_to=4 if x.shape[1] <= 4 else 8)
        t = EF.conv_bn_act(r, t, self.conv_stem, self.bn1, **_act_kw(False, self.act))
        wanted = {f['module'] for f in self.feature_info}
        feats = []
        for si, stage in enumerate(self.blocks):
            for bi, block in enumerate(stage):
                t = block(t)
                if all_features and f'blocks.{si}.{bi}' in wanted:
                    feats.append(t)
        if not all_features:
            feats.append(EF.conv_bn_act(r, t, self.conv_head, self.bn2, **_act_kw(False, self.act)))
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
    return _create_effnet(variant, pretrained, block_args=decode_arch_def(arch_def, _unsupported), stem_size=stem_size,
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


# ---- EfficientNet-Lite: no squeeze-excite, ReLU6, fixed stem and head -----------------------------------------------------
_EFFICIENTNET_LITE = [['ds_r1_k3_s1_e1_c16'], ['ir_r2_k3_s2_e6_c24'], ['ir_r2_k5_s2_e6_c40'], ['ir_r3_k3_s2_e6_c80'],
                      ['ir_r3_k5_s1_e6_c112'], ['ir_r4_k5_s2_e6_c192'], ['ir_r1_k3_s1_e6_c320']]


def _gen_efficientnet_lite(variant, channel_multiplier=1.0, depth_multiplier=1.0, pretrained=False, **kwargs):
    def round_chs_fn(c):
        return round_channels(c, multiplier=channel_multiplier)
    kwargs.setdefault('act_layer', 'relu6')
    block_args = decode_arch_def(_EFFICIENTNET_LITE, _unsupported, depth_multiplier=depth_multiplier, fix_first_last=True)
    return _create_effnet(variant, pretrained, block_args=block_args, num_features=1280, stem_size=32, fix_stem=True,
                          round_chs_fn=round_chs_fn, **kwargs)


def _lite_entry(name, channel_multiplier, depth_multiplier):
    def entry(pretrained=False, **kwargs):
        return _gen_efficientnet_lite(name, channel_multiplier, depth_multiplier, pretrained, **kwargs)
    entry.__name__ = entry.__qualname__ = name
    entry.__doc__ = (f'EfficientNet-Lite{name[-1]}: channel multiplier {channel_multiplier}, depth multiplier {depth_multiplier} '
                     f'(efficientnet.py:1528-1569)')
    return BACKBONES.register_class(entry)


efficientnet_lite0 = _lite_entry('efficientnet_lite0', 1.0, 1.0)
efficientnet_lite1 = _lite_entry('efficientnet_lite1', 1.0, 1.1)
efficientnet_lite2 = _lite_entry('efficientnet_lite2', 1.1, 1.2)
efficientnet_lite3 = _lite_entry('efficientnet_lite3', 1.2, 1.4)
efficientnet_lite4 = _lite_entry('efficientnet_lite4', 1.4, 1.8)
