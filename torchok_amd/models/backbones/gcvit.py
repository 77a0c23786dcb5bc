"""Global Context ViT backbones (``gcvit_*``) on the MI355X engine.

Mirrors ``torchok/models/backbones/gcvit.py``: ``GlobalContextVit`` (constructor signature and defaults, ``init_weights`` with
its two schemes, ``no_weight_decay``, ``forward_features``, ``forward``, ``load_state_dict`` honouring
``load_relative_position_bias_table``, ``get_stages``) and the five entry points, with the [timm 0.6.13] ``gcvit`` pieces the
reference imports (``Stem``, ``GlobalContextVitStage`` and what they are built from) restated here.  timm is not installed, so
the restatement was written from memory of timm 0.6.13.  Checked: with the reference's five configurations and a
``512 * embed_dim / 64 * 1000 + 1000`` parameter head it gives timm's published 12.00 / 19.98 / 28.22 / 51.09 / 90.32 M
parameters, and ``stem.conv1``, ``stages.N``, ``relative_position_bias_table`` and ``rel_pos`` are fixed by the reference file.
Resting on memory alone: the other key names, the ``repeat`` of the global query and the ``make_divisible`` rounding of the
squeeze-excite width (c / 4 at every width of the five variants).  tests/gcvit_ref.py is the same restatement in plain torch;
state dicts interchange with it both ways.

The global query.  Every second block of a stage attends with a query that does not come from its tokens: the stage computes
one (B, ws, ws, C) map ``q_global`` from its input (``global_block``) and the reference tiles it over the windows with
``q_global.repeat(B_windows // B, 1, 1, 1)``.  ``window_partition`` numbers windows image-major, ``repeat`` tiles image-minor,
so window u reads the query of image u mod B, not of its own image u div nW.  That is the reference's behaviour and parity is
the contract: the kernel reproduces it (``query_image`` in csrc/gc_attn.hip).  The two agree where nW == 1 or B == 1.

Execution: convolutional parts (stem, downsample, global_block) on NHWC maps, blocks on the token rows of the same buffer
(zero-copy reshape).  LayerNorm2d is the row LayerNorm kernel on the NHWC rows; MbConvBlock is depthwise 3x3 (no bias) -> GELU
-> squeeze-excite with GELU inside and no biases (tok_se_act_*) -> 1x1 -> residual; attention is ``gc_window_attention``
(csrc/gc_attn.hip) between the qkv and proj GEMMs with the bias gathered from the block's table (``relpos_bias``); residuals
are ``layer_scale_add`` (small / base) or ``residual_add`` with the drop-path row scales.  The backbone is one autograd node.

Not served (NotImplementedError, never a silent fallback): dropout (``drop_rate`` / ``proj_drop_rate`` / ``attn_drop_rate``
> 0), activations other than ``gelu``, norms other than ``layernorm2d`` / ``layernorm``, head_dim != 32, non-square windows, a
token map that is not a multiple of its window or whose global_block does not end on one window, more than 256 tokens per
window.
"""
import math
from functools import partial
from typing import Any, List, Mapping, Optional, Tuple

import torch
import torch.nn as nn

from ... import engine
from ...constructor import BACKBONES
from ...engine import functional as EF
from ...engine import transformer as ET
from ..base import BaseBackbone
from .swin import DropPath, Mlp, _scale_of, draw_drop_scales


def make_divisible(v, divisor=8, min_value=None, round_limit=.9):
    min_value = min_value or divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < round_limit * v:
        new_v += divisor
    return new_v


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class LayerNorm2d(nn.LayerNorm):
    """[timm 0.6.13] LayerNorm2d: LayerNorm over the channels of a map; here the row kernel on the NHWC rows."""

    def run(self, r, x):
        return ET.layer_norm(r, x, self)


class SEModule(nn.Module):
    """[timm 0.6.13] SEModule as MbConvBlock builds it: fc1 / fc2 without bias, GELU inside, sigmoid gate."""

    def __init__(self, channels: int, rd_ratio: float = 0.25):
        super().__init__()
        rd = make_divisible(channels * rd_ratio, 8, round_limit=0.)
        self.fc1 = nn.Conv2d(channels, rd, 1, bias=False)
        self.bn = nn.Identity()
        self.act = nn.GELU()
        self.fc2 = nn.Conv2d(rd, channels, 1, bias=False)
        self.gate = nn.Sigmoid()

    def run(self, r, x):
        return EF.squeeze_excite(r, x, self, gate='sigmoid', act='gelu', names=('fc1', 'fc2'))


class MbConvBlock(nn.Module):
    """x + conv_pw(se(gelu(conv_dw(x))))"""

    def __init__(self, c: int):
        super().__init__()
        self.conv_dw = nn.Conv2d(c, c, 3, 1, 1, groups=c, bias=False)
        self.act = nn.GELU()
        self.se = SEModule(c)
        self.conv_pw = nn.Conv2d(c, c, 1, 1, 0, bias=False)

    def run(self, r, x):
        y = ET.activation(r, ET.dwconv3x3(r, x, self.conv_dw), ET.GELU)
        y = EF.conv_bn_act(r, self.se.run(r, y), self.conv_pw, None)
        return ET.residual_add(r, x, y)


class Downsample2d(nn.Module):
    def __init__(self, dim: int, dim_out: Optional[int] = None, norm_layer=LayerNorm2d):
        super().__init__()
        dim_out = dim_out or dim
        self.norm1 = norm_layer(dim)
        self.conv_block = MbConvBlock(dim)
        self.reduction = nn.Conv2d(dim, dim_out, 3, 2, 1, bias=False)
        self.norm2 = norm_layer(dim_out)

    def run(self, r, x):
        x = self.conv_block.run(r, self.norm1.run(r, x))
        return self.norm2.run(r, EF.conv_bn_act(r, x, self.reduction, None))


class Stem(nn.Module):
    def __init__(self, in_chs: int, out_chs: int, norm_layer=LayerNorm2d):
        super().__init__()
        self.conv1 = nn.Conv2d(in_chs, out_chs, 3, 2, 1)
        self.down = Downsample2d(out_chs, norm_layer=norm_layer)

    def run(self, r, image: torch.Tensor):
        t = r.input(image, c_pad_to=4 if image.shape[1] <= 4 else 8)
        return self.down.run(r, EF.conv_bn_act(r, t, self.conv1, None))


class _Pool(nn.MaxPool2d):
    def run(self, r, x):
        return EF.max_pool_3x3_s2(r, x)


class FeatureBlock(nn.Module):
    """max(1, levels) MbConvBlocks, each of the first `levels` followed by MaxPool2d(3, 2, 1)"""

    def __init__(self, dim: int, levels: int = 0):
        super().__init__()
        reductions = levels
        self.blocks = nn.Sequential()
        for i in range(max(1, levels)):
            self.blocks.add_module(f'conv{i + 1}', MbConvBlock(dim))
            if reductions:
                self.blocks.add_module(f'pool{i + 1}', _Pool(3, 2, 1))
                reductions -= 1

    def run(self, r, x):
        for m in self.blocks:
            x = m.run(r, x)
        return x


def gen_relative_position_index(window_size: Tuple[int, int]) -> torch.Tensor:
    """Swin's relative position index without a class token: int64 [N][N]"""
    wh, ww = window_size
    coords = torch.stack(torch.meshgrid([torch.arange(wh), torch.arange(ww)], indexing='ij')).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += wh - 1
    rel[:, :, 1] += ww - 1
    rel[:, :, 0] *= 2 * ww - 1
    return rel.sum(-1).contiguous()


class RelPosBias(nn.Module):
    """[timm 0.6.13] layers.RelPosBias without prefix tokens: the table is a parameter, the index a non-persistent buffer."""

    def __init__(self, window_size: Tuple[int, int], num_heads: int):
        super().__init__()
        self.window_size = window_size
        self.num_heads = num_heads
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window_size[0] - 1) * (2 * window_size[1] - 1), num_heads))
        self.register_buffer('relative_position_index', gen_relative_position_index(window_size), persistent=False)
        self._index_checked = {}     # the engine's record of the index it has range-checked (no parameter, no buffer)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)


class WindowAttentionGlobal(nn.Module):
    """softmax((q * scale) k^T + bias) v per window; use_global: qkv holds k and v only and q is the stage's q_global."""

    def __init__(self, dim: int, num_heads: int, window_size: Tuple[int, int], use_global: bool = True, qkv_bias: bool = True,
                 attn_drop: float = 0., proj_drop: float = 0.):
        super().__init__()
        if dim % num_heads or dim // num_heads != 32:
            raise NotImplementedError(f'torchok_amd GCViT: head_dim 32 only (dim {dim}, {num_heads} heads)')
        if attn_drop > 0. or proj_drop > 0.:
            raise NotImplementedError('torchok_amd GCViT: attention / projection dropout')
        window_size = _pair(window_size)
        if window_size[0] != window_size[1]:
            raise NotImplementedError(f'torchok_amd GCViT: square windows (got {window_size})')
        if window_size[0] * window_size[1] > 256:
            raise NotImplementedError(f'torchok_amd GCViT: {window_size[0] * window_size[1]} tokens per window (at most 256)')
        self.window_size, self.num_heads, self.dim = window_size, num_heads, dim
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.use_global = use_global
        self.rel_pos = RelPosBias(window_size=window_size, num_heads=num_heads)
        self.qkv = nn.Linear(dim, dim * (2 if use_global else 3), bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def run(self, r, x, batch: int, size: Tuple[int, int], q_global):
        h, w = size
        ws = self.window_size[0]
        qkv = ET.linear_module(r, x, self.qkv)
        rp = self.rel_pos
        bias = ET.relpos_bias(r, rp.relative_position_bias_table, rp.relative_position_index, self.num_heads, ws * ws,
                              rp._index_checked)
        a = ET.gc_window_attention(r, qkv, (batch, h, w, self.dim, self.num_heads, ws), bias,
                                   q_global if self.use_global else None)
        return ET.linear_module(r, a, self.proj)


class LayerScale(nn.Module):
    def __init__(self, dim: int, init_values: float = 1e-5):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))


class GlobalContextVitBlock(nn.Module):
    """x = x + drop_path(ls1(attn(norm1(x), q_global)));  x = x + drop_path(ls2(mlp(norm2(x))))"""

    def __init__(self, dim: int, num_heads: int, window_size, mlp_ratio: float = 4., use_global: bool = True, qkv_bias: bool = True,
                 layer_scale: Optional[float] = None, proj_drop: float = 0., attn_drop: float = 0., drop_path: float = 0.,
                 norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttentionGlobal(dim, num_heads, window_size, use_global=use_global, qkv_bias=qkv_bias,
                                          attn_drop=attn_drop, proj_drop=proj_drop)
        self.ls1 = LayerScale(dim, layer_scale) if layer_scale is not None else nn.Identity()
        self.drop_path1 = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), drop=proj_drop)
        self.ls2 = LayerScale(dim, layer_scale) if layer_scale is not None else nn.Identity()
        self.drop_path2 = DropPath(drop_path) if drop_path > 0. else nn.Identity()

    def run(self, r, x, batch: int, size: Tuple[int, int], q_global):
        dev = x.data.device
        tokens = size[0] * size[1]
        a = self.attn.run(r, ET.layer_norm(r, x, self.norm1), batch, size, q_global)
        s1, s2 = _scale_of(self.drop_path1, batch, dev), _scale_of(self.drop_path2, batch, dev)
        if isinstance(self.ls1, LayerScale):
            x = ET.layer_scale_add(r, x, a, self.ls1.gamma, s1, tokens)
            return ET.layer_scale_add(r, x, self.mlp.run(r, ET.layer_norm(r, x, self.norm2)), self.ls2.gamma, s2, tokens)
        x = ET.residual_add(r, x, a, s1, tokens)
        return ET.residual_add(r, x, self.mlp.run(r, ET.layer_norm(r, x, self.norm2)), s2, tokens)


class GlobalContextVitStage(nn.Module):
    def __init__(self, dim: int, depth: int, num_heads: int, feat_size: Tuple[int, int], window_size: Tuple[int, int],
                 downsample: bool = True, stage_norm: bool = False, mlp_ratio: float = 4., qkv_bias: bool = True,
                 layer_scale: Optional[float] = None, proj_drop: float = 0., attn_drop: float = 0., drop_path=0.,
                 norm_layer=LayerNorm2d, norm_layer_cl=nn.LayerNorm):
        super().__init__()
        if downsample:
            self.downsample = Downsample2d(dim, dim * 2, norm_layer=norm_layer)
            dim = dim * 2
            feat_size = (feat_size[0] // 2, feat_size[1] // 2)
        else:
            self.downsample = nn.Identity()
        self.feat_size = feat_size
        window_size = _pair(window_size)
        self.window_size = window_size
        if feat_size[0] % window_size[0] or feat_size[1] % window_size[1]:
            raise NotImplementedError(f'torchok_amd GCViT: a {feat_size[0]}x{feat_size[1]} token map is not a multiple of the '
                                      f'window {window_size}')
        feat_levels = int(math.log2(min(feat_size) / min(window_size)))
        self.global_block = FeatureBlock(dim, feat_levels)
        self.global_norm = nn.Identity()
        drop_path = list(drop_path) if isinstance(drop_path, (list, tuple)) else [drop_path] * depth
        self.blocks = nn.ModuleList([
            GlobalContextVitBlock(dim, num_heads, window_size, mlp_ratio=mlp_ratio, use_global=(i % 2 != 0), qkv_bias=qkv_bias,
                                  layer_scale=layer_scale, proj_drop=proj_drop, attn_drop=attn_drop, drop_path=drop_path[i],
                                  norm_layer=norm_layer_cl) for i in range(depth)])
        self.norm = norm_layer_cl(dim) if stage_norm else nn.Identity()
        self.dim = dim

    def run(self, r, x):
        """x: a (B, H, W, C) map -> the stage's (B, H', W', C') map"""
        if isinstance(self.downsample, Downsample2d):
            x = self.downsample.run(r, x)
        batch, h, w, cp = x.shape
        ws = self.window_size[0]
        if h % ws or w % ws:
            raise NotImplementedError(f'torchok_amd GCViT: a {h}x{w} token map is not a multiple of the window {ws}')
        q_global = self.global_block.run(r, x)
        if tuple(q_global.shape[1:3]) != (ws, ws):
            raise NotImplementedError(f'torchok_amd GCViT: global_block leaves a {q_global.shape[1]}x{q_global.shape[2]} query map '
                                      f'for windows of {ws}x{ws} (the token map must be the window times a power of two)')
        t = ET.reshape(r, x, (batch * h * w, cp))
        for blk in self.blocks:
            t = blk.run(r, t, batch, (h, w), q_global)
        if isinstance(self.norm, nn.LayerNorm):
            t = ET.layer_norm(r, t, self.norm)
        return ET.reshape(r, t, (batch, h, w, cp))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """NCHW in, NCHW out: the stage on its own (a channels-last bf16 input may require grad)"""
        with engine.region() as r:
            if self.training:
                draw_drop_scales([p for blk in self.blocks for p in (blk.drop_path1, blk.drop_path2)], x.shape[0], x.device)
            return r.output(self.run(r, r.input(x)))


_NORMS_2D = {'layernorm2d': LayerNorm2d}
_NORMS_CL = {'layernorm': nn.LayerNorm}


class GlobalContextVit(BaseBackbone):
    """gcvit.py:46-184 (same constructor signature and defaults)."""

    def __init__(self, in_channels: int = 3, img_size: Tuple[int, int] = 224, window_ratio: Tuple[int, ...] = (32, 32, 16, 32),
                 window_size: Tuple[int, ...] = None, embed_dim: int = 64, depths: Tuple[int, ...] = (3, 4, 19, 5),
                 num_heads: Tuple[int, ...] = (2, 4, 8, 16), mlp_ratio: float = 3.0, qkv_bias: bool = True,
                 layer_scale: Optional[float] = None, drop_rate: float = 0., proj_drop_rate: float = 0., attn_drop_rate: float = 0.,
                 drop_path_rate: float = 0., weight_init='', act_layer: str = 'gelu', norm_layer: str = 'layernorm2d',
                 norm_layer_cl: str = 'layernorm', norm_eps: float = 1e-5, load_relative_position_bias_table: bool = True):
        num_stages = len(depths)
        super().__init__(in_channels=in_channels, out_channels=int(embed_dim * 2 ** (num_stages - 1)))
        if drop_rate > 0. or proj_drop_rate > 0. or attn_drop_rate > 0.:
            raise NotImplementedError('torchok_amd GCViT: dropout (drop_rate / proj_drop_rate / attn_drop_rate)')
        if act_layer != 'gelu':
            raise NotImplementedError(f'torchok_amd GCViT: activation {act_layer!r} (gelu only)')
        if norm_layer not in _NORMS_2D or norm_layer_cl not in _NORMS_CL:
            raise NotImplementedError(f'torchok_amd GCViT: norms {norm_layer!r} / {norm_layer_cl!r} (layernorm2d / layernorm only)')
        self.encoder_channels = [int(embed_dim * 2 ** i) for i in range(num_stages)]
        self._out_encoder_channels = self.encoder_channels
        self.load_relative_position_bias_table = load_relative_position_bias_table
        n2d = partial(_NORMS_2D[norm_layer], eps=norm_eps)
        ncl = partial(_NORMS_CL[norm_layer_cl], eps=norm_eps)
        img_size = _pair(img_size)
        feat_size = tuple(d // 4 for d in img_size)        # the stem reduces by 4
        self.img_size = img_size
        self.drop_rate = drop_rate
        if window_size is not None:
            window_size = tuple(window_size) if isinstance(window_size, (tuple, list)) else (window_size,) * num_stages
            window_size = tuple(_pair(w) for w in window_size)
        else:
            assert window_ratio is not None
            ratios = tuple(window_ratio) if isinstance(window_ratio, (tuple, list)) else (window_ratio,) * num_stages
            window_size = tuple((img_size[0] // r, img_size[1] // r) for r in ratios)
        self.stem = Stem(in_chs=in_channels, out_chs=embed_dim, norm_layer=n2d)
        dpr = [x.tolist() for x in torch.linspace(0, drop_path_rate, sum(depths), device='cpu').split(list(depths))]
        stages = []
        for i in range(num_stages):
            sc = 2 ** max(i - 1, 0)
            stages.append(GlobalContextVitStage(
                dim=embed_dim * sc, depth=depths[i], num_heads=num_heads[i], feat_size=(feat_size[0] // sc, feat_size[1] // sc),
                window_size=window_size[i], downsample=i != 0, stage_norm=i == num_stages - 1, mlp_ratio=mlp_ratio,
                qkv_bias=qkv_bias, layer_scale=layer_scale, proj_drop=proj_drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[i],
                norm_layer=n2d, norm_layer_cl=ncl))
        self.stages = nn.Sequential(*stages)
        self.init_weights(scheme=weight_init)

    def init_weights(self, scheme=''):
        """gcvit.py:122-139: 'vit': Linear weights Xavier-uniform, biases zero (Mlp biases N(0, 1e-6)); otherwise Linear weights
        N(0, .02) with zero biases.  Convolutions keep torch's default initialisation."""
        if any(p.is_meta for p in self.parameters()):
            return
        for name, m in self.named_modules():
            if not isinstance(m, nn.Linear):
                continue
            if scheme == 'vit':
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    if 'mlp' in name:
                        nn.init.normal_(m.bias, std=1e-6)
                    else:
                        nn.init.zeros_(m.bias)
            else:
                nn.init.normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {k for k, _ in self.named_parameters() if any(n in k for n in ('relative_position_bias_table', 'rel_pos.mlp'))}

    @torch.jit.ignore
    def group_matcher(self, coarse=False):
        return dict(stem=r'^stem', blocks=r'^stages\.(\d+)')

    def _run(self, r, x: torch.Tensor):
        if self.training:
            draw_drop_scales([p for st in self.stages for blk in st.blocks for p in (blk.drop_path1, blk.drop_path2)],
                             x.shape[0], x.device)
        t = self.stem.run(r, x)
        feats = []
        for st in self.stages:
            t = st.run(r, t)
            feats.append(t)
        return feats

    def forward_features(self, x: torch.Tensor) -> List[torch.Tensor]:
        """[x, s0, s1, s2, s3]: the image and every stage's NCHW map"""
        with engine.region() as r:
            outs = r.output(*self._run(r, x))
        return [x] + (list(outs) if isinstance(outs, tuple) else [outs])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """NCHW [B, 8E, H/32, W/32]"""
        with engine.region() as r:
            return r.output(self._run(r, x)[-1])

    def load_state_dict(self, state_dict: Mapping[str, Any], strict: bool = True):
        if not self.load_relative_position_bias_table:
            state_dict = {k: v for k, v in state_dict.items() if 'relative_position_bias_table' not in k}
        return super().load_state_dict(state_dict, strict)

    def get_stages(self, stage: int) -> nn.Module:
        """the stem and the first `stage` stages (gcvit.py:176-184)"""
        return nn.ModuleList([self.stem, *self.stages[:stage]])


def _create_gcvit(variant: str, pretrained: bool = False, **kwargs):
    # [timm 0.6.13] build_model_with_cfg with kwargs_filter: num_classes / global_pool / in_chans are dropped
    for k in ('num_classes', 'global_pool', 'in_chans'):
        kwargs.pop(k, None)
    if pretrained:
        raise RuntimeError(f'{variant}: pretrained weights need a download (no network here); pass '
                           f'pretrained=false and use task.load_checkpoint for local checkpoints')
    return GlobalContextVit(**kwargs)


GCVIT_VARIANTS = {
    'gcvit_xxtiny': dict(depths=(2, 2, 6, 2), num_heads=(2, 4, 8, 16)),
    'gcvit_xtiny': dict(depths=(3, 4, 6, 5), num_heads=(2, 4, 8, 16)),
    'gcvit_tiny': dict(depths=(3, 4, 19, 5), num_heads=(2, 4, 8, 16)),
    'gcvit_small': dict(depths=(3, 4, 19, 5), num_heads=(3, 6, 12, 24), embed_dim=96, mlp_ratio=2, layer_scale=1e-5),
    'gcvit_base': dict(depths=(3, 4, 19, 5), num_heads=(4, 8, 16, 32), embed_dim=128, mlp_ratio=2, layer_scale=1e-5),
}


def _entry(variant: str):
    def build(pretrained: bool = False, **kwargs):
        # (the reference's dict(..., **kwargs) raises TypeError on a repeated key; here a keyword overrides the default)
        return _create_gcvit(variant, pretrained=pretrained, **dict(GCVIT_VARIANTS[variant], **kwargs))
    build.__name__ = build.__qualname__ = variant
    build.__doc__ = f'{variant} (gcvit.py entry point of the same name)'
    return build


for _name in GCVIT_VARIANTS:
    globals()[_name] = BACKBONES.register_class(_entry(_name))
