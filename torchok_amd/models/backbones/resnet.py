"""ResNet backbones on the MI355X engine.

Mirrors the reference wiring ``torchok/models/backbones/resnet.py``: ``make_blocks`` (:363-405),
``ResNet.__init__`` (:462-526), ``init_weights`` (:529-539), ``forward`` (:541-551), ``get_stages``
(:553-563) and the ``resnet18/34/50/101/152`` entrypoints (:589-594, :648-653 ...), with the
[timm 0.6.13] ``BasicBlock`` / ``Bottleneck`` / ``downsample_conv`` semantics restated here
(SURVEY.md App. A.1).  Module / parameter names are those of timm, so reference checkpoints load.

Execution differs completely: each ``conv -> bn -> (+shortcut) -> relu`` group is ONE engine unit
(implicit-GEMM MFMA conv with BatchNorm statistics in its epilogue, one fused normalise/add/ReLU
pass), activations stay NHWC bf16 in HBM between units, and the whole backbone is a single
autograd node.  The nn.Conv2d / nn.BatchNorm2d children are parameter containers only.

output_stride 8 / 16 (every entry point with convolutional shortcuts): the dilated stages run in phase layout, EF.phase_split, on
the same units as the plain network (csrc/phase.hip is the only device code of their own).
drop_path_rate (stochastic depth, resnet.py:369-400): block i of the network's N gets DropPath(drop_path_rate * i / (N - 1)), none
where that is 0; the per-sample keep / scale vector (swin.DropPath, all of a step's vectors drawn at once in ResNet._run) is the
`row_scale` of the block's last unit, out = relu(s[sample] * bn(conv(.)) + shortcut) on csrc/bn_droppath.hip.  BatchNorm sees the
un-dropped convolution output, as in [timm 0.6.13], and a dropped sample still receives the batch-statistics terms of the
gradient.  A block with a rate takes the plain conv + BatchNorm apply for that unit, never the fused residual unit.  In eval mode or
at rate 0 the network is launch for launch the one without the argument.  drop_block_rate stays refused (timm's DropBlock cannot
be checked offline), and so does drop_path_rate with attn_layer='eca' (the channel-attention residual kernel has no row scale).
Only the plain (v1.5) family is built: no SE / anti-aliasing / drop-block
(plus the other plain-architecture entrypoints at the end of the file, the d / t stems, the ResNeXts of group width
4 ... 64 on the grouped 3x3 unit and the ECA-ResNets on the channel-attention residual unit, EF.eca_residual; the s-stem, SE,
blur-pool and RS variants of the reference are outside the hot-path scope).
"""
import math
from typing import List

import torch
import torch.nn as nn

from ... import engine
from ...constructor import BACKBONES
from ...engine import functional as EF
from ..base import BaseBackbone
from .swin import DropPath, draw_drop_scales


def get_padding(kernel_size: int, stride: int, dilation: int = 1) -> int:
    return ((stride - 1) + dilation * (kernel_size - 1)) // 2


def eca_kernel_size(channels: int, gamma: int = 2, beta: int = 1) -> int:
    """[timm 0.6.13] EcaModule: the window grows with log2 of the channel count (256 ... 1024 -> 5, 2048 -> 7), at least 3."""
    t = int(abs(math.log(channels, 2) + beta) / gamma)
    return max(t if t % 2 else t + 1, 3)


class EcaModule(nn.Module):
    """Efficient channel attention ([timm 0.6.13] layers/eca.py): a k-tap convolution over the channel axis of the pooled map,
    sigmoid, and a per-channel product.  A parameter container: EF.eca_residual runs it together with the block's residual."""

    def __init__(self, channels: int):
        super().__init__()
        k = eca_kernel_size(channels)
        self.conv = nn.Conv1d(1, 1, kernel_size=k, padding=k // 2, bias=False)


def _attn(attn_layer, channels):
    """The block's `se` child: the ECA module or None (the block has refused every other attention layer, SE among them)."""
    return EcaModule(channels) if attn_layer == 'eca' else None


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, cardinality=1, base_width=64,
                 reduce_first=1, dilation=1, first_dilation=None, act_layer=nn.ReLU, norm_layer=nn.BatchNorm2d,
                 attn_layer=None, aa_layer=None, drop_block=None, drop_path=None):
        super().__init__()
        assert cardinality == 1 and base_width == 64, 'BasicBlock only supports cardinality=1, base_width=64'
        first_dilation = first_dilation or dilation
        _unsupported(eca_dilated=attn_layer == 'eca' and (dilation != 1 or first_dilation != 1),
                     attn_layer=attn_layer != 'eca' and attn_layer, aa_layer=aa_layer, drop_block=drop_block)
        _refuse_eca_drop_path(attn_layer, drop_path)
        first_planes = planes // reduce_first
        outplanes = planes * self.expansion
        self.conv1 = nn.Conv2d(inplanes, first_planes, kernel_size=3, stride=stride, padding=first_dilation,
                               dilation=first_dilation, bias=False)
        self.bn1 = norm_layer(first_planes)
        self.act1 = act_layer(inplace=True)
        self.conv2 = nn.Conv2d(first_planes, outplanes, kernel_size=3, padding=dilation, dilation=dilation, bias=False)
        self.bn2 = norm_layer(outplanes)
        self.se = _attn(attn_layer, outplanes)
        self.act2 = act_layer(inplace=True)
        self.downsample = downsample
        self.stride = stride
        self.drop_path = drop_path        # DropPath or None; no parameters: the state_dict is that of the block without it

    def zero_init_last(self):
        nn.init.zeros_(self.bn2.weight)

    def forward(self, x):
        r = engine.current_region()
        # a dilated stage runs in phase layout (EF.phase_split): every 3x3 takes its operand in the phase that equals its
        # dilation.  The stage's first block has conv1 at the previous dilation and conv2 at the stage's: the split sits
        # between them, and the block input is split for the 1x1 projection (its narrower side), so that the shortcut arrives
        # in the phase of the unit that adds it.  Without dilation every to_phase returns its argument.
        d1, d2 = self.conv1.dilation[0], self.conv2.dilation[0]
        x = EF.to_phase(r, x, d1)
        shortcut = self._shortcut(r, EF.to_phase(r, x, d2))
        y = EF.to_phase(r, EF.conv_bn_act(r, x, self.conv1, self.bn1, relu=True), d2)
        if self.se is not None:
            return EF.eca_residual(r, EF.conv_bn_act(r, y, self.conv2, self.bn2, relu=False), self.se, shortcut)
        return EF.conv_bn_act(r, y, self.conv2, self.bn2, relu=True, shortcut=shortcut, row_scale=_drop_scale(self.drop_path, y))

    def _shortcut(self, r, x):
        return _shortcut(r, x, self.downsample)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, cardinality=1, base_width=64,
                 reduce_first=1, dilation=1, first_dilation=None, act_layer=nn.ReLU, norm_layer=nn.BatchNorm2d,
                 attn_layer=None, aa_layer=None, drop_block=None, drop_path=None):
        super().__init__()
        first_dilation = first_dilation or dilation
        _unsupported(eca_dilated=attn_layer == 'eca' and (dilation != 1 or first_dilation != 1),
                     attn_layer=attn_layer != 'eca' and attn_layer, aa_layer=aa_layer, drop_block=drop_block)
        _refuse_eca_drop_path(attn_layer, drop_path)
        width = int(math.floor(planes * (base_width / 64)) * cardinality)
        first_planes = width // reduce_first
        outplanes = planes * self.expansion
        self.conv1 = nn.Conv2d(inplanes, first_planes, kernel_size=1, bias=False)
        self.bn1 = norm_layer(first_planes)
        self.act1 = act_layer(inplace=True)
        # cardinality > 1 (ResNeXt): a grouped 3x3, which conv_bn_act hands to the grouped unit (EF.gconv_bn_act)
        self.conv2 = nn.Conv2d(first_planes, width, kernel_size=3, stride=stride, padding=first_dilation, dilation=first_dilation,
                               groups=cardinality, bias=False)
        self.bn2 = norm_layer(width)
        self.act2 = act_layer(inplace=True)
        self.conv3 = nn.Conv2d(width, outplanes, kernel_size=1, bias=False)
        self.bn3 = norm_layer(outplanes)
        self.se = _attn(attn_layer, outplanes)
        self.act3 = act_layer(inplace=True)
        self.downsample = downsample
        self.stride = stride
        self.drop_path = drop_path        # DropPath or None; no parameters: the state_dict is that of the block without it

    def zero_init_last(self):
        nn.init.zeros_(self.bn3.weight)

    def forward(self, x):
        r = engine.current_region()
        # a dilated stage runs in phase layout (EF.phase_split), the whole block in the phase that equals conv2's dilation: the
        # stage's first block still in the previous phase, the split in front of the second.  Without dilation: x itself.
        x = EF.to_phase(r, x, self.conv2.dilation[0])
        y = EF.conv_bn_act(r, x, self.conv1, self.bn1, relu=True)
        y = EF.conv_bn_act(r, y, self.conv2, self.bn2, relu=True)
        # the projection is recorded LAST before the unit that adds it: in backward its (strided) data gradient then opens the
        # gradient of the block input and conv1's dense 1x1 data gradient closes it — the accumulate + ReLU-mask pass over the
        # whole tensor runs in the ring kernel's staged epilogue instead of the parity-class kernel's read-modify-write of
        # untouched pixels
        shortcut = _shortcut(r, x, self.downsample)
        if self.se is not None:
            return EF.eca_residual(r, EF.conv_bn_act(r, y, self.conv3, self.bn3, relu=False), self.se, shortcut)
        return EF.conv_bn_act(r, y, self.conv3, self.bn3, relu=True, shortcut=shortcut, row_scale=_drop_scale(self.drop_path, y))


def _drop_scale(drop_path, t):
    """The block's per-sample keep / scale vector for this step (None in eval mode or without a DropPath): `t` is the operand of
    the block's last unit, in phase layout d * d images per sample."""
    if drop_path is None:
        return None
    return drop_path.sample_scale(t.shape[0] // (t.phase * t.phase), t.data.device)


def _refuse_eca_drop_path(attn_layer, drop_path):
    if attn_layer == 'eca' and drop_path is not None:
        raise NotImplementedError('torchok_amd ResNet: drop_path with attn_layer=eca is not built (the channel-attention residual '
                                  'kernel, csrc/eca.hip, has no row scale)')


def _shortcut(r, x, downsample):
    """The block input, or its projection: an ``nn.Sequential(conv, bn)`` ([timm] downsample_conv, hrnet.py) or a ConvBnAct
    brick without activation (necks/classification/hrnet.py:62-69).  On the main stream: on a branch stream of its own it
    measured no gain on ResNet-50 B=256 (23.8 vs 23.7 ms/step), the main-stream kernels already fill the GPU."""
    if downsample is None:
        return x
    if hasattr(downsample, 'run'):
        return downsample.run(r, x)
    if len(downsample) == 3:       # [timm] downsample_avg: (AvgPool2d | Identity, 1x1 conv, norm)
        if isinstance(downsample[0], nn.AvgPool2d):
            x = EF.avg_pool_2x2(r, x)
        return EF.conv_bn_act(r, x, downsample[1], downsample[2], relu=False)
    return EF.conv_bn_act(r, x, downsample[0], downsample[1], relu=False)


def _unsupported(**flags):
    bad = [k for k, v in flags.items() if v]
    if bad:
        raise NotImplementedError(f'torchok_amd ResNet: {bad} not built (plain v1.5 ResNets only)')


def downsample_conv(in_channels, out_channels, kernel_size, stride=1, dilation=1, first_dilation=None,
                    norm_layer=None):
    norm_layer = norm_layer or nn.BatchNorm2d
    kernel_size = 1 if stride == 1 and dilation == 1 else kernel_size
    first_dilation = (first_dilation or dilation) if kernel_size > 1 else 1
    p = get_padding(kernel_size, stride, first_dilation)
    return nn.Sequential(
        nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=p, dilation=first_dilation,
                  bias=False),
        norm_layer(out_channels))


def downsample_avg(in_channels, out_channels, kernel_size, stride=1, dilation=1, first_dilation=None, norm_layer=None):
    """[timm] downsample_avg: 2x2 average pool (only where the block strides) -> 1x1 stride-1 conv -> norm."""
    norm_layer = norm_layer or nn.BatchNorm2d
    pool = nn.Identity()
    if stride != 1:
        if stride != 2 or dilation != 1:
            raise NotImplementedError('torchok_amd ResNet: avg_down with stride 2, no dilation')
        pool = nn.AvgPool2d(2, stride, ceil_mode=True, count_include_pad=False)
    return nn.Sequential(pool, nn.Conv2d(in_channels, out_channels, 1, stride=1, padding=0, bias=False),
                         norm_layer(out_channels))


def make_blocks(block_fn, channels, block_repeats, inplanes, reduce_first=1, output_stride=32,
                down_kernel_size=1, avg_down=False, drop_block_rate=0., drop_path_rate=0., **kwargs):
    # dilated stages (output_stride 8 / 16) run in phase layout on the plain kernels (EF.phase_split).  Not with avg_down: timm's
    # AvgPool2dSame of a dilated 'd' / 't' shortcut is not built; not with ECA: its per-image mean is not phase-agnostic
    if drop_block_rate:
        raise NotImplementedError(f'torchok_amd ResNet: drop_block_rate={drop_block_rate} is not built (DropBlock of [timm 0.6.13] '
                                  f'cannot be checked offline); drop_path_rate is')
    if drop_path_rate and kwargs.get('attn_layer') == 'eca':
        _refuse_eca_drop_path('eca', drop_path_rate)
    if output_stride != 32 and (avg_down or kwargs.get('attn_layer') == 'eca'):
        raise NotImplementedError(f'torchok_amd ResNet: output_stride={output_stride} with '
                                  f'{"avg_down" if avg_down else "attn_layer=eca"} is not built (dilated stages: convolutional '
                                  f'shortcuts, no channel attention)')
    no_downsample_stages = kwargs.pop('no_downsample_stages', [0])
    stages, feature_info = [], []
    net_num_blocks, net_block_idx = sum(block_repeats), 0
    net_stride = 4
    dilation = prev_dilation = 1
    for stage_idx, (planes, num_blocks) in enumerate(zip(channels, block_repeats)):
        stage_name = f'layer{stage_idx + 1}'
        stride = 1 if stage_idx in no_downsample_stages else 2
        if net_stride >= output_stride:          # resnet.py:376-380: the stage dilates instead of striding
            dilation *= stride
            stride = 1
        else:
            net_stride *= stride
        downsample = None
        if stride != 1 or inplanes != planes * block_fn.expansion:
            make = downsample_avg if avg_down else downsample_conv
            downsample = make(inplanes, planes * block_fn.expansion, kernel_size=down_kernel_size,
                              stride=stride, dilation=dilation, first_dilation=prev_dilation,
                              norm_layer=kwargs.get('norm_layer'))
        blocks = []
        for block_idx in range(num_blocks):
            block_dpr = drop_path_rate * net_block_idx / (net_num_blocks - 1)      # stochastic depth linear decay rule
            blocks.append(block_fn(inplanes, planes, stride if block_idx == 0 else 1,
                                   downsample if block_idx == 0 else None, reduce_first=reduce_first, dilation=dilation,
                                   first_dilation=prev_dilation, drop_path=DropPath(block_dpr) if block_dpr > 0. else None,
                                   **kwargs))
            prev_dilation = dilation
            inplanes = planes * block_fn.expansion
            net_block_idx += 1
        stages.append((stage_name, nn.Sequential(*blocks)))
        feature_info.append(dict(num_chs=inplanes, reduction=net_stride, module=stage_name))
    return stages, feature_info


class ResNet(BaseBackbone):
    def __init__(self, block, layers, in_channels=3, output_stride=32, cardinality=1, base_width=64,
                 stem_width=64, stem_type='', replace_stem_pool=False, block_reduce_first=1, down_kernel_size=1,
                 avg_down=False, act_layer=nn.ReLU, norm_layer=nn.BatchNorm2d, aa_layer=None, drop_path_rate=0.,
                 drop_block_rate=0., zero_init_last=True, block_args=None):
        super().__init__(in_channels=in_channels)
        block_args = block_args or dict()
        if output_stride not in (8, 16, 32):
            raise ValueError('`output_stride` must be in (8, 16, 32)')
        _unsupported(stem_type=stem_type not in ('', 'deep', 'deep_tiered'), replace_stem_pool=replace_stem_pool,
                     aa_layer=aa_layer, act_layer=act_layer is not nn.ReLU, norm_layer=norm_layer is not nn.BatchNorm2d)
        deep_stem = 'deep' in stem_type
        inplanes = stem_width * 2 if deep_stem else 64
        if deep_stem:      # three 3x3 convs (resnet.py:475-486): conv1 becomes a Sequential, bn1 / act1 follow its last conv
            stem_chs = (3 * (stem_width // 4), stem_width) if 'tiered' in stem_type else (stem_width, stem_width)
            self.conv1 = nn.Sequential(
                nn.Conv2d(in_channels, stem_chs[0], 3, stride=2, padding=1, bias=False), norm_layer(stem_chs[0]),
                act_layer(inplace=True),
                nn.Conv2d(stem_chs[0], stem_chs[1], 3, stride=1, padding=1, bias=False), norm_layer(stem_chs[1]),
                act_layer(inplace=True),
                nn.Conv2d(stem_chs[1], inplanes, 3, stride=1, padding=1, bias=False))
        else:
            self.conv1 = nn.Conv2d(in_channels, inplanes, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = norm_layer(inplanes)
        self.act1 = act_layer(inplace=True)
        self.feature_info = [dict(num_chs=inplanes, reduction=2, module='act1')]
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)

        channels = [64, 128, 256, 512]
        stage_modules, stage_feature_info = make_blocks(
            block, channels, layers, inplanes, cardinality=cardinality, base_width=base_width,
            output_stride=output_stride, reduce_first=block_reduce_first, avg_down=avg_down,
            down_kernel_size=down_kernel_size, act_layer=act_layer, norm_layer=norm_layer, aa_layer=aa_layer,
            drop_block_rate=drop_block_rate, drop_path_rate=drop_path_rate, **block_args)
        for stage in stage_modules:
            self.add_module(*stage)
        self.feature_info.extend(stage_feature_info)
        self._out_channels = 512 * block.expansion
        self.create_hooks()
        self.init_weights(zero_init_last=zero_init_last)
        # masters live in [k][r][s][c] order (what the MFMA packs and the wgrad kernel use);
        # logical shapes / state_dict are unchanged
        self.to(memory_format=torch.channels_last)

    def init_weights(self, zero_init_last=True):
        for n, m in self.named_modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        if zero_init_last:
            for m in self.modules():
                if hasattr(m, 'zero_init_last'):
                    m.zero_init_last()

    def _run(self, r, x: torch.Tensor, all_features: bool = True):
        if self.training:       # every block's keep / scale vector of this step in one draw
            draw_drop_scales([blk.drop_path for layer in (self.layer1, self.layer2, self.layer3, self.layer4) for blk in layer],
                             x.shape[0], x.device)
        t = r.input(x, c_pad_to=4 if x.shape[1] <= 4 else 8)
        feats = []
        last = self.conv1
        if isinstance(self.conv1, nn.Sequential):            # deep stem: two conv-bn-relu units in front of the last conv
            t = EF.conv_bn_act(r, t, self.conv1[0], self.conv1[1], relu=True)
            t = EF.conv_bn_act(r, t, self.conv1[3], self.conv1[4], relu=True)
            last = self.conv1[6]
        if all_features or not EF.FUSE_STEM_POOL:
            t = EF.conv_bn_act(r, t, last, self.bn1, relu=True)
            feats.append(t)                      # 'act1', the first entry of feature_info
            t = EF.max_pool_3x3_s2(r, t)
        else:
            # nobody asked for act1: bn1 + ReLU + max-pool in one pass, the 112 x 112 activated map is never stored
            t = EF.conv_bn_act(r, t, last, self.bn1, relu=True, pool=True)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            t = layer(t)
            feats.append(t)
        # a dilated stage leaves its map in phase layout and the next stage continues from that tensor; what is RETURNED is
        # merged: every feature (it then has two consumers), or the last map alone
        return [EF.from_phase(r, f) for f in feats] if all_features else feats[:-1] + [EF.from_phase(r, feats[-1])]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        with engine.region() as r:
            feats = self._run(r, x, all_features=False)
            return r.output(feats[-1])

    def forward_features(self, x: torch.Tensor) -> List[torch.Tensor]:
        with engine.region() as r:
            feats = self._run(r, x)
            outs = r.output(*feats)
        return [x] + list(outs)

    def get_stages(self, stage: int) -> nn.Module:
        output = [self.conv1, self.bn1, self.act1, self.maxpool]
        layers = [self.layer1, self.layer2, self.layer3, self.layer4]
        return nn.ModuleList(output + layers[:stage])


def _create_resnet(variant, pretrained=False, **kwargs):
    # [timm] build_model_with_cfg: drops kwargs_filter keys, instantiates, loads weights iff pretrained
    for k in ('num_classes', 'global_pool', 'in_chans'):
        kwargs.pop(k, None)
    if pretrained:
        raise RuntimeError(f'{variant}: pretrained weights need a download (no network here); pass '
                           f'pretrained=false and use task.load_checkpoint for local checkpoints')
    return ResNet(**kwargs)


@BACKBONES.register_class
def resnet18(pretrained=False, **kwargs):
    return _create_resnet('resnet18', pretrained, **dict(block=BasicBlock, layers=[2, 2, 2, 2], **kwargs))


@BACKBONES.register_class
def resnet34(pretrained=False, **kwargs):
    return _create_resnet('resnet34', pretrained, **dict(block=BasicBlock, layers=[3, 4, 6, 3], **kwargs))


@BACKBONES.register_class
def resnet50(pretrained=False, **kwargs):
    return _create_resnet('resnet50', pretrained, **dict(block=Bottleneck, layers=[3, 4, 6, 3], **kwargs))


@BACKBONES.register_class
def resnet101(pretrained=False, **kwargs):
    return _create_resnet('resnet101', pretrained, **dict(block=Bottleneck, layers=[3, 4, 23, 3], **kwargs))


@BACKBONES.register_class
def resnet152(pretrained=False, **kwargs):
    return _create_resnet('resnet152', pretrained, **dict(block=Bottleneck, layers=[3, 8, 36, 3], **kwargs))


# ---- further plain v1.5 entrypoints of the reference (same blocks, other depths / bottleneck widths; the tv_ / ssl_ /
# swsl_ names differ from their plain twins only in the pretrained weights they would download) ----------------------
def _plain(name, block, layers, doc, default_pretrained=False, **fixed):
    def entry(pretrained=default_pretrained, **kwargs):
        return _create_resnet(name, pretrained, **dict(block=block, layers=layers, **fixed, **kwargs))
    entry.__name__ = entry.__qualname__ = name
    entry.__doc__ = doc
    return BACKBONES.register_class(entry)


resnet26 = _plain('resnet26', Bottleneck, [2, 2, 2, 2], 'resnet.py:623-628')
resnet200 = _plain('resnet200', Bottleneck, [3, 24, 36, 3], 'resnet.py:707-712')
tv_resnet34 = _plain('tv_resnet34', BasicBlock, [3, 4, 6, 3], 'resnet.py:724-729')
tv_resnet50 = _plain('tv_resnet50', Bottleneck, [3, 4, 6, 3], 'resnet.py:732-737')
tv_resnet101 = _plain('tv_resnet101', Bottleneck, [3, 4, 23, 3], 'resnet.py:740-745')
tv_resnet152 = _plain('tv_resnet152', Bottleneck, [3, 8, 36, 3], 'resnet.py:748-753')
wide_resnet50_2 = _plain('wide_resnet50_2', Bottleneck, [3, 4, 6, 3], 'resnet.py:756-765 (bottleneck width x 2)', base_width=128)
wide_resnet101_2 = _plain('wide_resnet101_2', Bottleneck, [3, 4, 23, 3], 'resnet.py:768-776', base_width=128)
ssl_resnet18 = _plain('ssl_resnet18', BasicBlock, [2, 2, 2, 2], 'resnet.py:881-888', default_pretrained=True)
ssl_resnet50 = _plain('ssl_resnet50', Bottleneck, [3, 4, 6, 3], 'resnet.py:891-898', default_pretrained=True)
swsl_resnet18 = _plain('swsl_resnet18', BasicBlock, [2, 2, 2, 2], 'resnet.py:942-949', default_pretrained=True)
swsl_resnet50 = _plain('swsl_resnet50', Bottleneck, [3, 4, 6, 3], 'resnet.py:953-960', default_pretrained=True)
# 'd' = deep stem (three 3x3 convs, width 32) + average-pool shortcut projections; 't' = tiered deep stem (24, 32)
_D = dict(stem_width=32, stem_type='deep', avg_down=True)
_T = dict(stem_width=32, stem_type='deep_tiered', avg_down=True)
resnet18d = _plain('resnet18d', BasicBlock, [2, 2, 2, 2], 'resnet.py:597-603', **_D)
resnet34d = _plain('resnet34d', BasicBlock, [3, 4, 6, 3], 'resnet.py:614-620', **_D)
resnet26d = _plain('resnet26d', Bottleneck, [2, 2, 2, 2], 'resnet.py:640-645', **_D)
resnet26t = _plain('resnet26t', Bottleneck, [2, 2, 2, 2], 'resnet.py:631-637', **_T)
resnet50d = _plain('resnet50d', Bottleneck, [3, 4, 6, 3], 'resnet.py:656-662', **_D)
resnet50t = _plain('resnet50t', Bottleneck, [3, 4, 6, 3], 'resnet.py:665-671', **_T)
resnet101d = _plain('resnet101d', Bottleneck, [3, 4, 23, 3], 'resnet.py:682-687', **_D)
resnet152d = _plain('resnet152d', Bottleneck, [3, 8, 36, 3], 'resnet.py:698-704', **_D)
resnet200d = _plain('resnet200d', Bottleneck, [3, 24, 36, 3], 'resnet.py:715-721', **_D)
# ResNeXt: Bottleneck.conv2 is a grouped 3x3 (csrc/conv_group.hip serves group widths 4 ... 64: the 32x4d, 32x8d and 64x4d
# families).  The 32x16d / 32x32d / 32x48d entries of the reference need group widths up to 384 and stay unregistered.
_X4 = dict(cardinality=32, base_width=4)
_X8 = dict(cardinality=32, base_width=8)
resnext50_32x4d = _plain('resnext50_32x4d', Bottleneck, [3, 4, 6, 3], 'resnet.py:787-792', **_X4)
resnext50d_32x4d = _plain('resnext50d_32x4d', Bottleneck, [3, 4, 6, 3], 'resnet.py:795-802', **_X4, **_D)
resnext101_32x4d = _plain('resnext101_32x4d', Bottleneck, [3, 4, 23, 3], 'resnet.py:805-810', **_X4)
resnext101_32x8d = _plain('resnext101_32x8d', Bottleneck, [3, 4, 23, 3], 'resnet.py:813-818', **_X8)
resnext101_64x4d = _plain('resnext101_64x4d', Bottleneck, [3, 4, 23, 3], 'resnet.py:821-826', cardinality=64, base_width=4)
tv_resnext50_32x4d = _plain('tv_resnext50_32x4d', Bottleneck, [3, 4, 6, 3], 'resnet.py:829-834', **_X4)
ig_resnext101_32x8d = _plain('ig_resnext101_32x8d', Bottleneck, [3, 4, 23, 3], 'resnet.py:837-845', default_pretrained=True, **_X8)
ssl_resnext50_32x4d = _plain('ssl_resnext50_32x4d', Bottleneck, [3, 4, 6, 3], 'resnet.py:901-908', default_pretrained=True, **_X4)
ssl_resnext101_32x4d = _plain('ssl_resnext101_32x4d', Bottleneck, [3, 4, 23, 3], 'resnet.py:911-918', default_pretrained=True, **_X4)
ssl_resnext101_32x8d = _plain('ssl_resnext101_32x8d', Bottleneck, [3, 4, 23, 3], 'resnet.py:921-928', default_pretrained=True, **_X8)
swsl_resnext50_32x4d = _plain('swsl_resnext50_32x4d', Bottleneck, [3, 4, 6, 3], 'resnet.py:963-971', default_pretrained=True, **_X4)
swsl_resnext101_32x4d = _plain('swsl_resnext101_32x4d', Bottleneck, [3, 4, 23, 3], 'resnet.py:974-982', default_pretrained=True, **_X4)
swsl_resnext101_32x8d = _plain('swsl_resnext101_32x8d', Bottleneck, [3, 4, 23, 3], 'resnet.py:985-993', default_pretrained=True, **_X8)
# ECA: efficient channel attention behind the last BatchNorm of every block (csrc/eca.hip, EF.eca_residual)
_ECA = dict(block_args=dict(attn_layer='eca'))
ecaresnet26t = _plain('ecaresnet26t', Bottleneck, [2, 2, 2, 2], 'resnet.py:1008-1017', **_T, **_ECA)
ecaresnet50d = _plain('ecaresnet50d', Bottleneck, [3, 4, 6, 3], 'resnet.py:1020-1027', **_D, **_ECA)
ecaresnet50t = _plain('ecaresnet50t', Bottleneck, [3, 4, 6, 3], 'resnet.py:1030-1038', **_T, **_ECA)
ecaresnetlight = _plain('ecaresnetlight', Bottleneck, [1, 1, 11, 3], 'resnet.py:1041-1048', stem_width=32, avg_down=True, **_ECA)
ecaresnet101d = _plain('ecaresnet101d', Bottleneck, [3, 4, 23, 3], 'resnet.py:1051-1058', **_D, **_ECA)
ecaresnet200d = _plain('ecaresnet200d', Bottleneck, [3, 24, 36, 3], 'resnet.py:1061-1068', **_D, **_ECA)
ecaresnet269d = _plain('ecaresnet269d', Bottleneck, [3, 30, 48, 8], 'resnet.py:1071-1078', **_D, **_ECA)
ecaresnext26t_32x4d = _plain('ecaresnext26t_32x4d', Bottleneck, [2, 2, 2, 2], 'resnet.py:1081-1090', **_X4, **_T, **_ECA)
ecaresnext50t_32x4d = _plain('ecaresnext50t_32x4d', Bottleneck, [2, 2, 2, 2], 'resnet.py:1093-1101 (the reference builds it with the layers of the 26t)',
                             **_X4, **_T, **_ECA)
