"""The plain-torch dilated ResNet the build is compared with, composed from the oracle's own pieces: oracle.timm_min.BasicBlock /
Bottleneck / downsample_conv already take `dilation` and `first_dilation`, and oracle.torchok_ref.ResNet supplies the stem, the
initialisation and forward_features.  What is added is the stage rule of the reference's make_blocks (resnet.py:372-403):

    if net_stride >= output_stride: dilation *= stride; stride = 1          else: net_stride *= stride
    every block gets first_dilation=prev_dilation, and prev_dilation = dilation after a stage's first block

and constructors in the runtime dict oracle.torchok_ref.BACKBONES under '<name>/os<output_stride>', so that
oracle.torchok_ref.ClassificationModel builds them."""
import torch.nn as nn

import oracle.timm_min as TM
import oracle.torchok_ref as R
import resnext_ref as X


def make_blocks(block_fn, channels, block_repeats, inplanes, output_stride=32, **kwargs):
    stages, feature_info = [], []
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
            blocks.append(block_fn(inplanes, planes, stride if block_idx == 0 else 1, downsample if block_idx == 0 else None,
                                   dilation=dilation, first_dilation=prev_dilation, **kwargs))
            prev_dilation = dilation
            inplanes = planes * block_fn.expansion
        stages.append((f'layer{stage_idx + 1}', nn.Sequential(*blocks)))
        feature_info.append(dict(num_chs=inplanes, reduction=net_stride, module=f'layer{stage_idx + 1}'))
    return stages, feature_info


class ResNet(R.ResNet):
    """oracle.torchok_ref.ResNet with its four stages rebuilt by the rule above (same names, same order) and initialised anew."""

    def __init__(self, block, layers, output_stride=32, base_width=64, zero_init_last=True, in_channels=3):
        super().__init__(block, layers, in_channels=in_channels, zero_init_last=zero_init_last, base_width=base_width)
        if output_stride not in (8, 16, 32):
            raise ValueError('`output_stride` must be in (8, 16, 32)')
        stages, info = make_blocks(block, [64, 128, 256, 512], layers, 64, output_stride=output_stride, base_width=base_width)
        self.feature_info = [dict(num_chs=64, reduction=2, module='act1')] + info
        for name, stage in stages:
            setattr(self, name, stage)           # replaces the registered stage in place: the module order is unchanged
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


# name -> (block, layers, base_width)
SPECS = {
    'resnet18': (TM.BasicBlock, [2, 2, 2, 2], 64),
    'resnet26': (TM.Bottleneck, [2, 2, 2, 2], 64),
    'resnet50': (TM.Bottleneck, [3, 4, 6, 3], 64),
    'resnext50_32x4d': (X.SPECS['resnext50_32x4d'][0], [3, 4, 6, 3], 4),
}


def build(name, output_stride, **kw):
    block, layers, base_width = SPECS[name]
    return ResNet(block, layers, output_stride=output_stride, base_width=base_width, **kw)


def key(name, output_stride):
    return f'{name}/os{output_stride}'


for _n in SPECS:
    for _os in (8, 16, 32):
        R.BACKBONES.setdefault(key(_n, _os), lambda _n=_n, _os=_os, **kw: build(_n, _os, **kw))

# (stride, padding, dilation) of the 3x3s the rule gives, as the issue that asked for the dilated nets lists them:
# {(name, output_stride): {module path: triple}}; paths not listed in a dilated stage's later blocks follow `rest`
EXPECTED = {
    ('resnet50', 8): {'layer3.0.conv2': (1, 1, 1), 'layer3.1.conv2': (1, 2, 2), 'layer3.5.conv2': (1, 2, 2),
                      'layer4.0.conv2': (1, 2, 2), 'layer4.1.conv2': (1, 4, 4), 'layer4.2.conv2': (1, 4, 4),
                      'layer2.0.conv2': (2, 1, 1), 'layer3.0.downsample.0': (1, 0, 1), 'layer4.0.downsample.0': (1, 0, 1)},
    ('resnet50', 16): {'layer3.0.conv2': (2, 1, 1), 'layer3.1.conv2': (1, 1, 1), 'layer4.0.conv2': (1, 1, 1),
                       'layer4.1.conv2': (1, 2, 2), 'layer4.2.conv2': (1, 2, 2), 'layer4.0.downsample.0': (1, 0, 1)},
    ('resnet18', 8): {'layer3.0.conv1': (1, 1, 1), 'layer3.0.conv2': (1, 2, 2), 'layer3.1.conv1': (1, 2, 2),
                      'layer3.1.conv2': (1, 2, 2), 'layer4.0.conv1': (1, 2, 2), 'layer4.0.conv2': (1, 4, 4),
                      'layer4.1.conv1': (1, 4, 4), 'layer4.1.conv2': (1, 4, 4), 'layer3.0.downsample.0': (1, 0, 1),
                      'layer4.0.downsample.0': (1, 0, 1)},
    ('resnet18', 16): {'layer3.0.conv1': (2, 1, 1), 'layer3.1.conv2': (1, 1, 1), 'layer4.0.conv1': (1, 1, 1),
                       'layer4.0.conv2': (1, 2, 2), 'layer4.1.conv1': (1, 2, 2), 'layer4.1.conv2': (1, 2, 2)},
    ('resnext50_32x4d', 16): {'layer4.0.conv2': (1, 1, 1), 'layer4.1.conv2': (1, 2, 2), 'layer4.2.conv2': (1, 2, 2)},
}
REDUCTIONS = {8: [2, 4, 8, 8, 8], 16: [2, 4, 8, 16, 16], 32: [2, 4, 8, 16, 32]}
