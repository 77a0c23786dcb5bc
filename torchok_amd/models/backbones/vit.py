"""Vision Transformer backbones (``vit_*``) on the MI355X engine.

Mirrors ``torchok/models/backbones/vit.py``: ``VisionTransformer`` (:200-357: ``_pos_embed`` :284-298, ``forward_features``
:300-319, ``forward`` :321-329, ``get_stages`` :331-343) and the entry points (:426-887), with the [timm 0.6.13]
``vision_transformer`` pieces (PatchEmbed, Attention, Block, Mlp, ``init_weights_vit_timm``) restated here.  Module and
parameter names are timm's, so reference checkpoints load.

Execution: the tokens of every image stay one bf16 ``[B*T][D]`` matrix for the whole backbone.  The patch embedding is a
gather of the non-overlapping patches plus one GEMM (``engine.transformer.patch_embed``); the class token and the position
embedding are one launch (``vit_embed``); attention over all T tokens of an image reads q / k / v straight out of the qkv
GEMM's rows and writes the proj GEMM's input rows (``global_attention``, csrc/attn_global.hip); every Linear runs on the MFMA
GEMM kernels; the final norm runs on the B class-token rows only (LayerNorm is per row: ``norm(x)[:, 0] == norm(x[:, 0])``).
The backbone is one autograd node.

Not served (NotImplementedError, never a silent fallback): LayerScale (``init_values``), blocks other than ``Block``
(ParallelBlock, ResPostBlock), dropout (``drop_rate`` / ``attn_drop_rate`` > 0), head_dim != 64, weight_init schemes other
than '' and 'skip'.
"""
from functools import partial
from typing import List, Optional, Tuple, Union

import torch
import torch.nn as nn

from ... import engine
from ...constructor import BACKBONES
from ...engine import transformer as ET
from ..base import BaseBackbone
from .swin import DropPath, Mlp, _scale_of, draw_drop_scales, to_2tuple, trunc_normal_


class PatchEmbed(nn.Module):
    """[timm] layers.PatchEmbed with flatten=True and no norm: Conv2d(k = stride = patch)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, bias=True):
        super().__init__()
        self.img_size, self.patch_size = to_2tuple(img_size), to_2tuple(patch_size)
        if self.patch_size[0] != self.patch_size[1]:
            raise NotImplementedError('torchok_amd ViT: square patches')
        if self.img_size[0] % self.patch_size[0] or self.img_size[1] % self.patch_size[1]:
            raise NotImplementedError(f'torchok_amd ViT: img_size {self.img_size} is not a multiple of the patch size '
                                      f'{self.patch_size[0]}')
        if in_chans > 4:
            raise NotImplementedError('torchok_amd ViT: at most 4 input channels')
        self.grid_size = (self.img_size[0] // self.patch_size[0], self.img_size[1] // self.patch_size[1])
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.patch_size, bias=bias)
        self.norm = nn.Identity()

    def run(self, r, image: torch.Tensor):
        if tuple(image.shape[2:]) != self.img_size:
            raise ValueError(f'Input image size ({image.shape[2]}*{image.shape[3]}) doesn\'t match model '
                             f'({self.img_size[0]}*{self.img_size[1]}).')
        t = r.input(image, c_pad_to=4)
        rows, _ = ET.patch_embed(r, t, self.proj)
        return rows


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, attn_drop=0., proj_drop=0.):
        super().__init__()
        if dim % num_heads or dim // num_heads != 64:
            raise NotImplementedError(f'torchok_amd ViT: head_dim 64 only (embed_dim {dim}, {num_heads} heads)')
        if attn_drop > 0. or proj_drop > 0.:
            raise NotImplementedError('torchok_amd ViT: attention / projection dropout')
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def run(self, r, x, batch: int, tokens: int):
        qkv = ET.linear_module(r, x, self.qkv)
        a = ET.global_attention(r, qkv, batch, tokens, self.num_heads)
        return ET.linear_module(r, a, self.proj)


class Block(nn.Module):
    """[timm 0.6.13] vision_transformer.Block without LayerScale:
    x = x + drop_path1(attn(norm1(x)));  x = x + drop_path2(mlp(norm2(x)))."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0., init_values=None, drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        if init_values is not None:
            raise NotImplementedError('torchok_amd ViT: LayerScale (init_values)')
        if drop > 0.:
            raise NotImplementedError('torchok_amd ViT: dropout (drop_rate)')
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.ls1 = nn.Identity()
        self.drop_path1 = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.ls2 = nn.Identity()
        self.drop_path2 = DropPath(drop_path) if drop_path > 0. else nn.Identity()

    def run(self, r, x, batch: int, tokens: int):
        dev = x.data.device
        a = self.attn.run(r, ET.layer_norm(r, x, self.norm1), batch, tokens)
        x = ET.residual_add(r, x, a, _scale_of(self.drop_path1, batch, dev), tokens)
        m = self.mlp.run(r, ET.layer_norm(r, x, self.norm2))
        return ET.residual_add(r, x, m, _scale_of(self.drop_path2, batch, dev), tokens)


def _layer_norm_factory(norm_layer):
    """None -> timm's partial(nn.LayerNorm, eps=1e-6); nn.LayerNorm (eps 1e-5) or a partial of it as given."""
    if norm_layer is None:
        return partial(nn.LayerNorm, eps=1e-6)
    base = norm_layer.func if isinstance(norm_layer, partial) else norm_layer
    if base is not nn.LayerNorm:
        raise NotImplementedError('torchok_amd ViT: LayerNorm only')
    return norm_layer


class VisionTransformer(BaseBackbone):
    """vit.py:200-357 (same constructor signature)."""

    def __init__(self, img_size: Union[int, Tuple[int, int]] = 224, patch_size: int = 16, in_channels: int = 3,
                 embed_dim: int = 768, depth: int = 12, num_heads: int = 12, mlp_ratio: float = 4., qkv_bias: bool = True,
                 init_values: float = None, class_token=True, no_embed_class=False, pre_norm=False, drop_rate: float = 0.,
                 attn_drop_rate: float = 0., drop_path_rate: float = 0., weight_init: str = '', block_fn: nn.Module = Block,
                 embed_layer: nn.Module = PatchEmbed, norm_layer: nn.Module = None, act_layer: nn.Module = None):
        super().__init__(in_channels=in_channels, out_channels=embed_dim)
        if init_values is not None:
            raise NotImplementedError('torchok_amd ViT: LayerScale (init_values)')
        if block_fn is not Block:
            raise NotImplementedError('torchok_amd ViT: block_fn other than Block (ParallelBlock, ResPostBlock)')
        if embed_layer is not PatchEmbed:
            raise NotImplementedError('torchok_amd ViT: embed_layer other than PatchEmbed')
        if drop_rate > 0. or attn_drop_rate > 0.:
            raise NotImplementedError('torchok_amd ViT: dropout (drop_rate / attn_drop_rate)')
        if embed_dim % num_heads or embed_dim // num_heads != 64:
            raise NotImplementedError(f'torchok_amd ViT: head_dim 64 only (embed_dim {embed_dim}, {num_heads} heads)')
        if weight_init not in ('', 'skip'):
            raise NotImplementedError(f"torchok_amd ViT: weight_init '{weight_init}' ('' and 'skip' only)")
        if act_layer not in (None, nn.GELU):
            raise NotImplementedError('torchok_amd ViT: GELU')
        norm_layer = _layer_norm_factory(norm_layer)
        act_layer = act_layer or nn.GELU

        self.num_features = self.embed_dim = embed_dim
        self.num_prefix_tokens = 1 if class_token else 0
        self.no_embed_class = no_embed_class
        self.encoder_channels = [embed_dim] * 4
        self._out_encoder_channels = self.encoder_channels

        self.patch_embed = embed_layer(img_size=img_size, patch_size=patch_size, in_chans=in_channels, embed_dim=embed_dim,
                                       bias=not pre_norm)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim)) if class_token else None
        embed_len = num_patches if no_embed_class else num_patches + self.num_prefix_tokens
        self.pos_embed = nn.Parameter(torch.randn(1, embed_len, embed_dim) * .02)
        self.pos_drop = nn.Dropout(p=drop_rate)
        self.norm_pre = norm_layer(embed_dim) if pre_norm else nn.Identity()
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]     # stochastic depth decay rule (:259)
        self.blocks = nn.Sequential(*[
            block_fn(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, init_values=init_values,
                     drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[i], norm_layer=norm_layer, act_layer=act_layer)
            for i in range(depth)])
        self.norm = norm_layer(embed_dim)
        if weight_init != 'skip':
            self.init_weights(weight_init)

    def init_weights(self, mode=''):
        """init_weights('') of the reference: trunc_normal_(pos_embed, .02), cls_token ~ N(0, 1e-6), every nn.Linear
        trunc_normal_(.02) with a zero bias ([timm] init_weights_vit_timm); convolutions and LayerNorms keep torch's defaults."""
        if mode != '':
            raise NotImplementedError(f"torchok_amd ViT: weight_init '{mode}'")
        trunc_normal_(self.pos_embed, std=.02)
        if self.cls_token is not None:
            nn.init.normal_(self.cls_token, std=1e-6)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                trunc_normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'pos_embed', 'cls_token', 'dist_token'}

    def _tokens(self, r, x: torch.Tensor):
        """patch_embed -> _pos_embed -> norm_pre -> blocks (vit.py:300-307); -> token rows [B*T][D]."""
        batch = x.shape[0]
        t = self.patch_embed.run(r, x)
        t = ET.vit_embed(r, t, batch, self.pos_embed, self.cls_token, self.no_embed_class)
        if isinstance(self.norm_pre, nn.LayerNorm):
            t = ET.layer_norm(r, t, self.norm_pre)
        if self.training:
            draw_drop_scales([p for blk in self.blocks for p in (blk.drop_path1, blk.drop_path2)], batch, x.device)
        tokens = self.patch_embed.num_patches + self.num_prefix_tokens
        for blk in self.blocks:
            t = blk.run(r, t, batch, tokens)
        return t

    def forward_features(self, x: torch.Tensor) -> List[torch.Tensor]:
        """[x] + 4 x the (B, D, gh, gw) map of the last block's patch tokens, before `norm` (vit.py:300-319).  The reference
        drops one leading token unconditionally (x[:, 1:]); here the prefix tokens are dropped, which is the same thing with a
        class token and the only shape that reshapes without one."""
        batch = x.shape[0]
        gh, gw = self.patch_embed.grid_size
        with engine.region() as r:
            t = self._tokens(r, x)
            f = ET.rows_select(r, t, batch, self.num_prefix_tokens, gh * gw)
            f = r.output(ET.reshape(r, f, (batch, gh, gw, f.cp)))
        return [x] + [f] * 4

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """norm(x)[:, 0] (vit.py:321-329), with the norm on the B rows of token 0 only."""
        with engine.region() as r:
            t = self._tokens(r, x)
            first = ET.rows_select(r, t, x.shape[0], 0, 1)
            return r.output(ET.layer_norm(r, first, self.norm))

    def get_stages(self, stage: int) -> nn.Module:
        """vit.py:331-343, quirk included: the holder wraps pos_embed / cls_token in NEW nn.Parameter objects (sharing the
        storage), so freezing the returned stages leaves the model's own pos_embed / cls_token trainable."""
        holder = nn.Identity()
        holder.pos_embed = nn.Parameter(self.pos_embed)
        holder.cls_token = nn.Parameter(self.cls_token)
        output = [self.patch_embed, holder, self.pos_drop, self.norm_pre]
        return nn.ModuleList(output + list(self.blocks[:stage]))


def _create_vision_transformer(variant: str, pretrained: bool = False, **kwargs):
    # [timm 0.6.13] build_model_with_cfg: every _cfg here has fixed_input_size=True, so img_size defaults to the H, W of the
    # variant's input_size — (384, 384) for the *_384 entries (vit.py:42-200), (224, 224) for every other served entry
    # (the *_plus_* sizes, 256 / 240, are not served) — unless the caller passes img_size.  num_classes / global_pool / in_chans
    # are filtered out (kwargs_filter, :415).
    for k in ('num_classes', 'global_pool', 'in_chans'):
        kwargs.pop(k, None)
    if pretrained:
        raise RuntimeError(f'{variant}: pretrained weights need a download (no network here); pass '
                           f'pretrained=false and use task.load_checkpoint for local checkpoints')
    kwargs.setdefault('img_size', (384, 384) if variant.endswith('_384') else (224, 224))
    return VisionTransformer(**kwargs)


# name -> (patch, embed_dim, depth, heads, extra kwargs): the reference entry points whose default configuration is served
_TI, _S, _B, _L = (192, 12, 3), (384, 12, 6), (768, 12, 12), (1024, 24, 16)
_CLIP = dict(pre_norm=True, norm_layer=nn.LayerNorm)
VIT_VARIANTS = {
    'vit_tiny_patch16_224': (16, _TI, {}), 'vit_tiny_patch16_384': (16, _TI, {}),
    'vit_small_patch32_224': (32, _S, {}), 'vit_small_patch32_384': (32, _S, {}),
    'vit_small_patch16_224': (16, _S, {}), 'vit_small_patch16_384': (16, _S, {}),
    'vit_base_patch32_224': (32, _B, {}), 'vit_base_patch32_384': (32, _B, {}),
    'vit_base_patch16_224': (16, _B, {}), 'vit_base_patch16_384': (16, _B, {}),
    'vit_base_patch8_224': (8, _B, {}),
    'vit_large_patch32_224': (32, _L, {}), 'vit_large_patch32_384': (32, _L, {}),
    'vit_large_patch16_224': (16, _L, {}), 'vit_large_patch16_384': (16, _L, {}),
    'vit_large_patch14_224': (14, _L, {}),
    'vit_tiny_patch16_224_in21k': (16, _TI, {}), 'vit_small_patch32_224_in21k': (32, _S, {}),
    'vit_small_patch16_224_in21k': (16, _S, {}), 'vit_base_patch32_224_in21k': (32, _B, {}),
    'vit_base_patch16_224_in21k': (16, _B, {}), 'vit_base_patch8_224_in21k': (8, _B, {}),
    'vit_large_patch32_224_in21k': (32, _L, {}), 'vit_large_patch16_224_in21k': (16, _L, {}),
    'vit_base_patch16_224_sam': (16, _B, {}), 'vit_base_patch32_224_sam': (32, _B, {}),
    'vit_small_patch16_224_dino': (16, _S, {}), 'vit_small_patch8_224_dino': (8, _S, {}),
    'vit_base_patch16_224_dino': (16, _B, {}), 'vit_base_patch8_224_dino': (8, _B, {}),
    'vit_base_patch16_224_miil_in21k': (16, _B, dict(qkv_bias=False)),
    'vit_base_patch16_224_miil': (16, _B, dict(qkv_bias=False)),
    'vit_base_patch32_224_clip_laion2b': (32, _B, _CLIP),
    'vit_large_patch14_224_clip_laion2b': (14, _L, _CLIP),
}


def _entry(variant: str):
    patch, (dim, depth, heads), extra = VIT_VARIANTS[variant]

    def build(pretrained: bool = False, **kwargs):
        # (the reference's dict(..., **kwargs) raises TypeError on a repeated key; here a keyword overrides the default)
        model_kwargs = dict(dict(patch_size=patch, embed_dim=dim, depth=depth, num_heads=heads, **extra), **kwargs)
        return _create_vision_transformer(variant, pretrained=pretrained, **model_kwargs)
    build.__name__ = build.__qualname__ = variant
    build.__doc__ = f'{variant} (vit.py entry point of the same name)'
    return build


for _name in VIT_VARIANTS:
    globals()[_name] = BACKBONES.register_class(_entry(_name))
