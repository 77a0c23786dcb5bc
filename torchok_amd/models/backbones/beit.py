"""BEiT backbones (``beit_*``) on the MI355X engine.

Mirrors ``torchok/models/backbones/beit.py``: ``Beit`` (:61-203: ``fix_init_weight`` :120-126, ``init_weights`` :129-144,
``no_weight_decay`` :147-152, ``forward`` :181-192, ``get_stages`` :194-203) and the seven entry points (:213-273), with the
[timm 0.6.13] ``beit`` pieces (``gen_relative_position_index``, ``Attention``, ``Block``) restated here.  Module and parameter
names are timm's, so reference checkpoints load; ``fpn1`` ... ``fpn4`` exist as parameter containers for that reason
(``nn.BatchNorm2d`` stands in for ``nn.SyncBatchNorm`` under the same keys).

Execution: the token rows of ViT (vit.py) with the two things a BEiT block adds.  Attention adds a relative-position bias to
the scaled logits: the ``[heads][N][N]`` bias is gathered from the block's table (``engine.transformer.relpos_bias``), consumed
by the biased form of the global-attention kernel and dropped; the backward gathers it again, so no block keeps its bias across
the step.  The residuals are LayerScale residuals, ``x + drop_path(gamma * f(norm(x)))`` in one launch (``layer_scale_add``).
qkv has no bias of its own: ``cat(q_bias, 0, v_bias)`` rides the qkv GEMM and its gradient's first and last thirds go to
``q_bias`` / ``v_bias``.  The class token and ``pos_embed`` (with ``use_abs_pos_emb=False``: a zero buffer that takes no
gradient) are one launch; the final norm runs on the B class-token rows only.  The backbone is one autograd node.

Not served (NotImplementedError, never a silent fallback): ``forward_features`` (the FPN of transposed convolutions),
``use_shared_rel_pos_bias=True``, dropout (``drop_rate`` / ``attn_drop_rate`` > 0), head_dim != 64, norms other than LayerNorm.
"""
import logging
import math
from functools import partial
from typing import Tuple

import torch
import torch.nn as nn

from ... import engine
from ...constructor import BACKBONES
from ...engine import transformer as ET
from ..base import BaseBackbone
from .swin import DropPath, Mlp, _scale_of, draw_drop_scales, trunc_normal_
from .vit import PatchEmbed


def gen_relative_position_index(window_size: Tuple[int, int]) -> torch.Tensor:
    """[timm 0.6.13] beit.gen_relative_position_index: int64 [N][N], N = Wh * Ww + 1.  Patch-to-patch entries as in Swin;
    with T = (2 Wh - 1)(2 Ww - 1) + 3: row 0 (cls -> token) = T - 3, column 0 (token -> cls) = T - 2, [0][0] = T - 1."""
    wh, ww = window_size
    num_relative_distance = (2 * wh - 1) * (2 * ww - 1) + 3
    area = wh * ww
    coords = torch.stack(torch.meshgrid([torch.arange(wh), torch.arange(ww)], indexing='ij'))       # 2, Wh, Ww
    flat = torch.flatten(coords, 1)                                                                 # 2, Wh*Ww
    rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()                       # Wh*Ww, Wh*Ww, 2
    rel[:, :, 0] += wh - 1
    rel[:, :, 1] += ww - 1
    rel[:, :, 0] *= 2 * ww - 1
    index = torch.zeros((area + 1,) * 2, dtype=rel.dtype)
    index[1:, 1:] = rel.sum(-1)
    index[0, 0:] = num_relative_distance - 3
    index[0:, 0] = num_relative_distance - 2
    index[0, 0] = num_relative_distance - 1
    return index


class Attention(nn.Module):
    """[timm 0.6.13] beit.Attention: attn = softmax((q * scale) k^T + relative_position_bias)."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, attn_drop=0., proj_drop=0., window_size=None):
        super().__init__()
        if dim % num_heads or dim // num_heads != 64:
            raise NotImplementedError(f'torchok_amd BEiT: head_dim 64 only (embed_dim {dim}, {num_heads} heads)')
        if attn_drop > 0. or proj_drop > 0.:
            raise NotImplementedError('torchok_amd BEiT: attention / projection dropout')
        self.num_heads, self.dim = num_heads, dim
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=False)
        if qkv_bias:
            self.q_bias = nn.Parameter(torch.zeros(dim))
            self.register_buffer('k_bias', torch.zeros(dim), persistent=False)
            self.v_bias = nn.Parameter(torch.zeros(dim))
        else:
            self.q_bias = self.k_bias = self.v_bias = None
        if window_size:
            self.window_size = tuple(window_size)
            self.num_relative_distance = (2 * window_size[0] - 1) * (2 * window_size[1] - 1) + 3
            self.relative_position_bias_table = nn.Parameter(torch.zeros(self.num_relative_distance, num_heads))
            self.register_buffer('relative_position_index', gen_relative_position_index(self.window_size))
        else:
            self.window_size = None
            self.relative_position_bias_table = None
            self.relative_position_index = None
        self._index_checked = {}     # the engine's record of the index it has range-checked (no parameter, no buffer)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def run(self, r, x, batch: int, tokens: int):
        if self.q_bias is not None:
            qkv_bias = torch.cat((self.q_bias.detach(), self.k_bias, self.v_bias.detach()))
            qkv = ET.linear_op(r, x, self.qkv.weight, qkv_bias, [(self.q_bias, 0), (self.v_bias, 2 * self.dim)])
        else:
            qkv = ET.linear_op(r, x, self.qkv.weight)
        bias = None
        if self.relative_position_bias_table is not None:
            bias = ET.relpos_bias(r, self.relative_position_bias_table, self.relative_position_index, self.num_heads, tokens,
                                  self._index_checked)
        a = ET.global_attention(r, qkv, batch, tokens, self.num_heads, bias=bias)
        return ET.linear_module(r, a, self.proj)


class Block(nn.Module):
    """[timm 0.6.13] beit.Block:  x = x + drop_path(gamma_1 * attn(norm1(x)));  x = x + drop_path(gamma_2 * mlp(norm2(x)));
    without init_values a plain residual.  timm applies its one ``drop_path`` module twice (two independent draws); here the
    two draws have a module each (``drop_path1`` / ``drop_path2``, no parameters), as in vit.py, so that a step's keep/scale
    vectors come from one batched draw."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0., drop_path=0., init_values=None,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, window_size=None):
        super().__init__()
        if drop > 0.:
            raise NotImplementedError('torchok_amd BEiT: dropout (drop_rate)')
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop,
                              window_size=window_size)
        self.drop_path1 = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.drop_path2 = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        if init_values:
            self.gamma_1 = nn.Parameter(init_values * torch.ones(dim))
            self.gamma_2 = nn.Parameter(init_values * torch.ones(dim))
        else:
            self.gamma_1 = self.gamma_2 = None

    def run(self, r, x, batch: int, tokens: int):
        dev = x.data.device
        a = self.attn.run(r, ET.layer_norm(r, x, self.norm1), batch, tokens)
        s1, s2 = _scale_of(self.drop_path1, batch, dev), _scale_of(self.drop_path2, batch, dev)
        if self.gamma_1 is None:
            x = ET.residual_add(r, x, a, s1, tokens)
            return ET.residual_add(r, x, self.mlp.run(r, ET.layer_norm(r, x, self.norm2)), s2, tokens)
        x = ET.layer_scale_add(r, x, a, self.gamma_1, s1, tokens)
        return ET.layer_scale_add(r, x, self.mlp.run(r, ET.layer_norm(r, x, self.norm2)), self.gamma_2, s2, tokens)


def _layer_norm_factory(norm_layer):
    base = norm_layer.func if isinstance(norm_layer, partial) else norm_layer
    if base is not nn.LayerNorm:
        raise NotImplementedError('torchok_amd BEiT: LayerNorm only')
    return norm_layer


class Beit(BaseBackbone):
    """beit.py:61-203 (same constructor signature)."""

    def __init__(self, img_size=224, patch_size=16, in_channels=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.,
                 qkv_bias=True, drop_rate=0., attn_drop_rate=0., drop_path_rate=0., out_indices=(3, 5, 7, 11),
                 norm_layer=partial(nn.LayerNorm, eps=1e-6), init_values=None, use_abs_pos_emb=True,
                 use_rel_pos_bias=False, use_shared_rel_pos_bias=False):
        super().__init__(in_channels=in_channels)
        if use_shared_rel_pos_bias:
            raise NotImplementedError('torchok_amd BEiT: use_shared_rel_pos_bias (one table for all blocks)')
        if drop_rate > 0. or attn_drop_rate > 0.:
            raise NotImplementedError('torchok_amd BEiT: dropout (drop_rate / attn_drop_rate)')
        if embed_dim % num_heads or embed_dim // num_heads != 64:
            raise NotImplementedError(f'torchok_amd BEiT: head_dim 64 only (embed_dim {embed_dim}, {num_heads} heads)')
        norm_layer = _layer_norm_factory(norm_layer)
        self.num_features = embed_dim
        self.out_indices = out_indices
        self.encoder_channels = [embed_dim] * len(out_indices)
        self._out_channels = embed_dim
        self._out_encoder_channels = self.encoder_channels

        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_channels, embed_dim=embed_dim)
        self.img_size = self.patch_embed.img_size
        num_patches = self.patch_embed.num_patches

        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim)) if use_abs_pos_emb else None
        if not use_abs_pos_emb:
            # what the token-assembly launch adds in place of pos_embed: zeros that take no gradient (not in the state_dict)
            self.register_buffer('_zero_pos', torch.zeros(1, num_patches + 1, embed_dim), persistent=False)
        self.pos_drop = nn.Dropout(p=drop_rate)
        self.rel_pos_bias = None

        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth, device='cpu')]     # stochastic depth decay rule (:92)
        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop=drop_rate,
                  attn_drop=attn_drop_rate, drop_path=dpr[i], norm_layer=norm_layer, init_values=init_values,
                  window_size=self.patch_embed.grid_size if use_rel_pos_bias else None)
            for i in range(depth)])

        # parameter containers of forward_features' FPN (:100-114): never run here, their gradients stay None
        if patch_size == 16:
            self.fpn1 = nn.Sequential(nn.ConvTranspose2d(embed_dim, embed_dim, kernel_size=2, stride=2),
                                      nn.BatchNorm2d(embed_dim), nn.GELU(),
                                      nn.ConvTranspose2d(embed_dim, embed_dim, kernel_size=2, stride=2))
            self.fpn2 = nn.ConvTranspose2d(embed_dim, embed_dim, kernel_size=2, stride=2)
            self.fpn3 = nn.Identity()
            self.fpn4 = nn.MaxPool2d(kernel_size=2, stride=2)
        elif patch_size == 8:
            self.fpn1 = nn.ConvTranspose2d(embed_dim, embed_dim, kernel_size=2, stride=2)
            self.fpn2 = nn.Identity()
            self.fpn3 = nn.MaxPool2d(kernel_size=2, stride=2)
            self.fpn4 = nn.MaxPool2d(kernel_size=4, stride=4)

        self.norm = norm_layer(embed_dim)
        self.init_weights()

    def fix_init_weight(self):
        for layer_id, layer in enumerate(self.blocks):
            layer.attn.proj.weight.data.div_(math.sqrt(2.0 * (layer_id + 1)))
            layer.mlp.fc2.weight.data.div_(math.sqrt(2.0 * (layer_id + 1)))

    @torch.jit.ignore
    def init_weights(self):
        """beit.py:129-144: every nn.Linear trunc_normal_(.02) with a zero bias, LayerNorms (1, 0), pos_embed and cls_token
        trunc_normal_(.02), then fix_init_weight; tables stay zero and gammas init_values."""
        if any(p.is_meta for p in self.parameters()):
            return
        for m in self.modules():
            if isinstance(m, nn.Linear):
                trunc_normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)
        if self.pos_embed is not None:
            trunc_normal_(self.pos_embed, std=.02)
        trunc_normal_(self.cls_token, std=.02)
        self.fix_init_weight()

    @torch.jit.ignore
    def no_weight_decay(self):
        nwd = {'pos_embed', 'cls_token'}
        for n, _ in self.named_parameters():
            if 'relative_position_bias_table' in n:
                nwd.add(n)
        return nwd

    def forward_features(self, x):
        raise NotImplementedError('torchok_amd BEiT: forward_features (the FPN of transposed convolutions over the out_indices '
                                  'blocks is not built); forward() serves classification')

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """norm(x)[:, 0][..., None, None] (beit.py:181-192), with the norm on the B rows of token 0 only."""
        batch = x.shape[0]
        with engine.region() as r:
            t = self.patch_embed.run(r, x)
            pos = self.pos_embed if self.pos_embed is not None else self._zero_pos
            t = ET.vit_embed(r, t, batch, pos, self.cls_token)
            if self.training:
                draw_drop_scales([p for blk in self.blocks for p in (blk.drop_path1, blk.drop_path2)], batch, x.device)
            tokens = self.patch_embed.num_patches + 1
            for blk in self.blocks:
                t = blk.run(r, t, batch, tokens)
            first = ET.rows_select(r, t, batch, 0, 1)
            out = r.output(ET.layer_norm(r, first, self.norm))
        return out[..., None, None]

    def get_stages(self, stage: int) -> nn.Module:
        """beit.py:194-203: the whole model, with the reference's warning."""
        logging.warning('BEIT does not support `get_stages`. Return the whole model')
        return self


def _create_beit(variant: str, pretrained: bool = False, **kwargs):
    # [timm 0.6.13] build_model_with_cfg with kwargs_filter (:207): num_classes / global_pool / in_chans are dropped
    for k in ('num_classes', 'global_pool', 'in_chans'):
        kwargs.pop(k, None)
    if pretrained:
        raise RuntimeError(f'{variant}: pretrained weights need a download (no network here); pass '
                           f'pretrained=false and use task.load_checkpoint for local checkpoints')
    return Beit(**kwargs)


_BASE = dict(patch_size=16, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, use_abs_pos_emb=False, use_rel_pos_bias=True,
             init_values=0.1)
_LARGE = dict(patch_size=16, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4, qkv_bias=True, use_abs_pos_emb=False,
              use_rel_pos_bias=True, init_values=1e-5)
BEIT_VARIANTS = {
    'beit_base_patch16_224': _BASE, 'beit_base_patch16_384': dict(_BASE, img_size=384), 'beit_base_patch16_224_in22k': _BASE,
    'beit_large_patch16_224': _LARGE, 'beit_large_patch16_384': dict(_LARGE, img_size=384),
    'beit_large_patch16_512': dict(_LARGE, img_size=512), 'beit_large_patch16_224_in22k': _LARGE,
}


def _entry(variant: str):
    def build(pretrained: bool = False, **kwargs):
        # (the reference's dict(..., **kwargs) raises TypeError on a repeated key; here a keyword overrides the default)
        return _create_beit(variant, pretrained=pretrained, **dict(BEIT_VARIANTS[variant], **kwargs))
    build.__name__ = build.__qualname__ = variant
    build.__doc__ = f'{variant} (beit.py entry point of the same name)'
    return build


for _name in BEIT_VARIANTS:
    globals()[_name] = BACKBONES.register_class(_entry(_name))
