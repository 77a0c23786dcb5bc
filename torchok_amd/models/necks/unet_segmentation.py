"""UnetNeck (reference ``torchok/models/necks/segmentation/unet.py:20-131``): the U-Net decoder over the feature pyramid of
any backbone with ``forward_features``.  Centre block (two 3x3 ConvBnReLU) on the deepest map, then per decoder block a
nearest x2 upsample, channel concat with the skip of that level (resized to the upsampled map when its height differs) and
two 3x3 ConvBnReLU.  Here the upsample, the resize and the concat are one engine unit (engine/resample.py: nearest_concat
writes every source straight into its channel slice) and every ConvBnAct is one fused conv-BN-ReLU unit.
Served: the reference's default configuration.  ``use_attention=True`` (SCSE) and ``use_batchnorm=False`` are refused."""
from typing import List, Sequence

import torch.nn as nn
from torch import Tensor

from ... import engine
from ...constructor import NECKS
from ...engine import resample as ER
from ..base import BaseModel
from ..modules import ConvBnAct


class DecoderBlock(nn.Module):
    def __init__(self, in_channels: int, skip_channels: int, out_channels: int, use_attention: bool = False,
                 use_batchnorm: bool = True):
        super().__init__()
        if use_attention:
            raise NotImplementedError('torchok_amd UnetNeck: use_attention=True (SCSE attention) is not built')
        in_channels = in_channels + skip_channels
        self.attention1 = nn.Identity()
        self.conv1 = ConvBnAct(in_channels, out_channels, kernel_size=3, padding=1, use_batchnorm=use_batchnorm)
        self.conv2 = ConvBnAct(out_channels, out_channels, kernel_size=3, padding=1, use_batchnorm=use_batchnorm)
        self.attention2 = nn.Identity()

    def run(self, region, x, skip=None):
        size = (2 * x.shape[1], 2 * x.shape[2])
        # unet.py:50 compares the heights only: a skip of the same height and another width fails in torch.cat there
        if skip is not None and skip.shape[1] == size[0] and skip.shape[2] != size[1]:
            raise ValueError(f'UnetNeck: skip map {skip.shape[1:3]} has the height of the upsampled map {size} but not its width')
        x = ER.nearest_concat(region, [x] if skip is None else [x, skip], size)
        return self.conv2.run(region, self.conv1.run(region, x))


class CenterBlock(nn.Sequential):
    def __init__(self, in_channels: int, out_channels: int, use_batchnorm: bool = True):
        super().__init__(ConvBnAct(in_channels, out_channels, kernel_size=3, padding=1, use_batchnorm=use_batchnorm),
                         ConvBnAct(out_channels, out_channels, kernel_size=3, padding=1, use_batchnorm=use_batchnorm))

    def run(self, region, x):
        return self[1].run(region, self[0].run(region, x))


@NECKS.register_class
class UnetNeck(BaseModel):
    def __init__(self, in_channels: Sequence[int], decoder_channels: Sequence[int] = (512, 256, 128, 64, 64),
                 use_batchnorm: bool = True, use_attention: bool = False, center: bool = True):
        super().__init__(in_channels=in_channels, out_channels=decoder_channels[-1])
        self.n_blocks = len(decoder_channels)
        encoder_channels = list(in_channels)[::-1]          # start from the head of the encoder
        head_channels = encoder_channels[0]
        block_in = [head_channels] + list(decoder_channels[:-1])
        skip_channels = encoder_channels[1:] + [0]
        self.center = CenterBlock(head_channels, head_channels, use_batchnorm) if center else nn.Identity()
        self.blocks = nn.ModuleList([DecoderBlock(i, s, o, use_attention=use_attention, use_batchnorm=use_batchnorm)
                                     for i, s, o in zip(block_in, skip_channels, decoder_channels)])
        self.init_weights()

    def forward(self, features: List[Tensor]) -> List[Tensor]:
        head, *skips, input_image = features[::-1]
        with engine.region() as r:
            x = r.input(head)
            if isinstance(self.center, CenterBlock):
                x = self.center.run(r, x)
            for i, block in enumerate(self.blocks):
                x = block.run(r, x, r.input(skips[i]) if i < len(skips) else None)
            out = r.output(x)
        return [input_image, out]
