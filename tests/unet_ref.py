"""Plain-torch fp32 statement of the U-Net segmentation neck (reference torchok/models/necks/segmentation/unet.py with
use_attention=False): what torchok_amd's UnetNeck must compute, with the reference's child names so state_dicts interchange.
tests/golden/unet_neck.npz pins it to the reference's own code bit for bit (tests/test_unet_ref.py).  SegmentationModel
composes it with the oracle's ResNet-18 and the segmentation head, under the child names of SegmentationTask."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import oracle.hrnet_ref as H
import oracle.torchok_ref as R


class ConvBnRelu(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size=3, padding=1, bias=False)
        self.bn = nn.BatchNorm2d(cout)
        self.act = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.act(self.bn(self.conv(x)))


class DecoderBlock(nn.Module):
    def __init__(self, cin, cskip, cout):
        super().__init__()
        self.attention1 = nn.Identity()
        self.conv1 = ConvBnRelu(cin + cskip, cout)
        self.conv2 = ConvBnRelu(cout, cout)
        self.attention2 = nn.Identity()

    def forward(self, x, skip=None):
        x = F.interpolate(x, scale_factor=2, mode='nearest')
        if skip is not None:
            if skip.size(2) != x.size(2):          # heights only
                skip = F.interpolate(skip, size=x.shape[2:], mode='nearest')
            x = torch.cat([x, skip], dim=1)
        return self.conv2(self.conv1(x))


class UnetNeck(nn.Module):
    def __init__(self, in_channels, decoder_channels=(512, 256, 128, 64, 64), center=True):
        super().__init__()
        enc = list(in_channels)[::-1]
        ins = [enc[0]] + list(decoder_channels[:-1])
        skips = enc[1:] + [0]
        self.out_channels = decoder_channels[-1]
        self.center = nn.Sequential(ConvBnRelu(enc[0], enc[0]), ConvBnRelu(enc[0], enc[0])) if center else nn.Identity()
        self.blocks = nn.ModuleList(DecoderBlock(i, s, o) for i, s, o in zip(ins, skips, decoder_channels))

    def forward(self, features):
        head, *skips, image = features[::-1]
        x = self.center(head)
        for i, block in enumerate(self.blocks):
            x = block(x, skips[i] if i < len(skips) else None)
        return [image, x]


class SegmentationModel(nn.Module):
    """resnet18 -> UnetNeck -> SegmentationHead (tasks/segmentation.py:60-93)."""

    def __init__(self, num_classes, decoder_channels=(512, 256, 128, 64, 64), **backbone_kw):
        super().__init__()
        self.backbone = R.resnet18(**backbone_kw)
        self.neck = UnetNeck((64, 64, 128, 256, 512), decoder_channels)
        self.head = nn.Module()
        self.head.classifier = nn.Conv2d(self.neck.out_channels, num_classes, kernel_size=1)
        self.num_classes = num_classes

    head_forward = H.SegmentationModel.head_forward

    def forward_with_gt(self, batch):
        feats = self.backbone.forward_features(batch['image'])
        return {'prediction': self.head_forward(self.neck(feats)), 'target': batch['target']}
