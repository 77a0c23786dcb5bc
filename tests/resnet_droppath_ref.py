"""The plain-torch ResNet with stochastic depth the build is compared with, composed from the oracle's own pieces:
oracle.timm_min.BasicBlock / Bottleneck already take a `drop_path` child and apply it to the last BatchNorm output, in front of the
residual add (timm_min.py:66-75, 105-115).  What is added is the rate rule of the reference's make_blocks (resnet.py:369-400),

    block_dpr = drop_path_rate * net_block_idx / (net_num_blocks - 1)
    drop_path = DropPath(block_dpr) if block_dpr > 0. else None

on top of the stage rule restated in tests/dilated_ref.py (output_stride 8 / 16 / 32), and a DropPath whose per-sample factors can
be PINNED, so that a run of the build and a run of the restatement drop the same samples.  Constructors land in the runtime
dict oracle.torchok_ref.BACKBONES under '<name>/os<output_stride>/droppath' and take `drop_path_rate`."""
import torch
import torch.nn as nn

import dilated_ref as DR
import oracle.timm_min as TM
import oracle.torchok_ref as R


class PinnedDropPath(TM.DropPath):
    """[timm 0.6.13] DropPath; `pinned` (a [B] vector of factors, 0 or 1 / keep) replaces the draw while it is set"""
    pinned = None

    def forward(self, x):
        if self.drop_prob == 0. or not self.training:
            return x
        if self.pinned is None:
            return super().forward(x)
        return x * self.pinned.to(x.dtype).view(-1, *([1] * (x.ndim - 1)))


def block_rates(block_repeats, drop_path_rate):
    n = sum(block_repeats)
    return [drop_path_rate * i / (n - 1) for i in range(n)]


def make_blocks(block_fn, channels, block_repeats, inplanes, output_stride=32, drop_path_rate=0., **kwargs):
    stages, feature_info = [], []
    net_num_blocks, net_block_idx = sum(block_repeats), 0
    net_stride = 4
    dilation = prev_dilation = 1
    for stage_idx, (planes, num_blocks) in enumerate(zip(channels, block_repeats)):
        stride = 1 if stage_idx == 0 else 2
        if net_stride >= output_stride:
            dilation *= stride
            stride = 1
        else:
            net_stride *= stride
        downsample = None
        if stride != 1 or inplanes != planes * block_fn.expansion:
            downsample = TM.downsample_conv(inplanes, planes * block_fn.expansion, kernel_size=1, stride=stride,
                                            dilation=dilation, first_dilation=prev_dilation)
        blocks = []
        for block_idx in range(num_blocks):
            block_dpr = drop_path_rate * net_block_idx / (net_num_blocks - 1)
            blocks.append(block_fn(inplanes, planes, stride if block_idx == 0 else 1, downsample if block_idx == 0 else None,
                                   dilation=dilation, first_dilation=prev_dilation,
                                   drop_path=PinnedDropPath(block_dpr) if block_dpr > 0. else None, **kwargs))
            prev_dilation = dilation
            inplanes = planes * block_fn.expansion
            net_block_idx += 1
        stages.append((f'layer{stage_idx + 1}', nn.Sequential(*blocks)))
        feature_info.append(dict(num_chs=inplanes, reduction=net_stride, module=f'layer{stage_idx + 1}'))
    return stages, feature_info


class ResNet(R.ResNet):
    """oracle.torchok_ref.ResNet with its four stages rebuilt by the rules above (same names, same order) and initialised anew."""

    def __init__(self, block, layers, output_stride=32, drop_path_rate=0., base_width=64, zero_init_last=True, in_channels=3):
        super().__init__(block, layers, in_channels=in_channels, zero_init_last=zero_init_last, base_width=base_width)
        stages, _ = make_blocks(block, [64, 128, 256, 512], layers, 64, output_stride=output_stride, drop_path_rate=drop_path_rate,
                                base_width=base_width)
        for name, stage in stages:
            setattr(self, name, stage)
            for m in stage.modules():
                if isinstance(m, nn.Conv2d):
                    nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                elif isinstance(m, nn.BatchNorm2d):
                    nn.init.ones_(m.weight)
                    nn.init.zeros_(m.bias)
            if zero_init_last:
                for m in stage.modules():
                    if hasattr(m, 'zero_init_last'):
                        m.zero_init_last()


def blocks_of(backbone):
    return [blk for layer in (backbone.layer1, backbone.layer2, backbone.layer3, backbone.layer4) for blk in layer]


def key(name, output_stride=32):
    return f'{name}/os{output_stride}/droppath'


for _n, (_block, _layers, _bw) in DR.SPECS.items():
    for _os in (8, 16, 32):
        R.BACKBONES.setdefault(key(_n, _os), lambda _b=_block, _l=_layers, _w=_bw, _os=_os, **kw: ResNet(
            _b, _l, output_stride=_os, base_width=_w, **kw))


def pinned_scales(rates, batch, seed, drop=(), keep_all=()):
    """One [batch] vector of factors per block (None where the rate is 0): sample i of block k is kept where a seeded uniform
    draw is >= the block's rate.  drop = ((block, sample), ...) forces a drop, keep_all = (block, ...) keeps every sample."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k, rate in enumerate(rates):
        if rate <= 0:
            out.append(None)
            continue
        keep = (torch.rand(batch, generator=g) >= rate).float()
        if k in keep_all:
            keep.fill_(1.0)
        for kk, i in drop:
            if kk == k:
                keep[i] = 0.0
        out.append((keep / (1.0 - rate)).float())
    return out


def pin(blocks, scales, device=None):
    """hand every block its vector: the restatement's PinnedDropPath.pinned, or the build's DropPath._drawn (consumed by the
    block's next forward, so a step of the build is pinned anew)"""
    for blk, s in zip(blocks, scales):
        if s is None:
            assert blk.drop_path is None
        elif isinstance(blk.drop_path, PinnedDropPath):
            blk.drop_path.pinned = s.clone()
        else:
            blk.drop_path._drawn = s.clone().to(device)
