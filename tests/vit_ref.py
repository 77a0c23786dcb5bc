"""Plain-torch fp32 restatement of the reference Vision Transformer (torchok/models/backbones/vit.py:200-357 on
[timm 0.6.13] vision_transformer Attention / Block / Mlp / PatchEmbed): the oracle of tests/test_vit*.py.  Module names are
timm's, so state_dicts load both ways.  It lives under tests/ because oracle/ is frozen and the reference imports timm."""
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F


class PatchEmbed(nn.Module):
    def __init__(self, img_size, patch_size, in_chans, embed_dim, bias=True):
        super().__init__()
        self.img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
        self.grid_size = (self.img_size[0] // patch_size, self.img_size[1] // patch_size)
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.proj = nn.Conv2d(in_chans, embed_dim, patch_size, patch_size, bias=bias)

    def forward(self, x):
        return self.proj(x).flatten(2).transpose(1, 2)


class Attention(nn.Module):
    def __init__(self, dim, num_heads, qkv_bias):
        super().__init__()
        self.num_heads = num_heads
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.unbind(0)
        attn = (q @ k.transpose(-2, -1)) * (C // self.num_heads) ** -0.5
        attn = attn.softmax(dim=-1)
        return self.proj((attn @ v).transpose(1, 2).reshape(B, N, C))


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio, qkv_bias, norm_layer):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads, qkv_bias)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))
        self.drop_scales = None       # (scale1, scale2) per-sample vectors: stochastic depth with pinned draws

    def forward(self, x):
        s1, s2 = self.drop_scales or (None, None)
        a = self.attn(self.norm1(x))
        x = x + (a if s1 is None else a * s1[:, None, None])
        m = self.mlp(self.norm2(x))
        return x + (m if s2 is None else m * s2[:, None, None])


class VisionTransformer(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_channels=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.,
                 qkv_bias=True, class_token=True, no_embed_class=False, pre_norm=False, norm_layer=None):
        super().__init__()
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        self.num_prefix_tokens = 1 if class_token else 0
        self.no_embed_class = no_embed_class
        self.patch_embed = PatchEmbed(img_size, patch_size, in_channels, embed_dim, bias=not pre_norm)
        n = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim)) if class_token else None
        self.pos_embed = nn.Parameter(torch.randn(1, n if no_embed_class else n + self.num_prefix_tokens, embed_dim) * .02)
        self.norm_pre = norm_layer(embed_dim) if pre_norm else nn.Identity()
        self.blocks = nn.Sequential(*[Block(embed_dim, num_heads, mlp_ratio, qkv_bias, norm_layer) for _ in range(depth)])
        self.norm = norm_layer(embed_dim)

    def _pos_embed(self, x):
        if self.no_embed_class:
            x = x + self.pos_embed
            if self.cls_token is not None:
                x = torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1)
        else:
            if self.cls_token is not None:
                x = torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1)
            x = x + self.pos_embed
        return x

    def tokens(self, x):
        return self.blocks(self.norm_pre(self._pos_embed(self.patch_embed(x))))

    def forward_features(self, x):
        t = self.tokens(x)[:, self.num_prefix_tokens:].permute(0, 2, 1)
        return [x] + [t.reshape(t.shape[0], t.shape[1], *self.patch_embed.grid_size)] * 4

    def forward(self, x):
        return self.norm(self.tokens(x))[:, 0]


class Classifier(nn.Module):
    """ClassificationTask(backbone, head=ClassificationHead) without pooling: backbone.* / head.fc.*."""

    def __init__(self, num_classes, **kwargs):
        super().__init__()
        self.backbone = VisionTransformer(**kwargs)
        self.head = nn.Module()
        self.head.fc = nn.Linear(self.backbone.norm.normalized_shape[0], num_classes)

    def forward(self, x):
        return self.head.fc(self.backbone(x))
