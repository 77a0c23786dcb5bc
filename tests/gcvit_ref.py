"""The Global Context ViT of [timm 0.6.13] ``gcvit`` restated in plain torch (timm is not installed), and the arithmetic of the
window-attention kernel's contract (csrc/gc_attn.hip).

The restatement was written from memory of timm 0.6.13.  What is checked: built with the reference's five entry-point
configurations and ``512 * embed_dim / 64 * 1000 + 1000`` head parameters added it gives timm's published 12.00 / 19.98 /
28.22 / 51.09 / 90.32 M parameters (tests/test_gcvit_ref.py holds the backbone counts), and ``stem.conv1``, ``stages.N``,
``relative_position_bias_table`` and ``rel_pos`` are fixed by the reference's backbone file.  What rests on memory alone: the
other key names, the ``repeat`` of the global query (image-minor: window u takes the query of image u mod B), and the
``make_divisible`` rounding of the squeeze-excite width (c / 4 at every width of the five variants).

Use ``.double()`` on a model for an fp64 run.
"""
import math
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

HD = 32
SCALE = HD ** -0.5


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def make_divisible(v, divisor=8, min_value=None, round_limit=.9):
    min_value = min_value or divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < round_limit * v:
        new_v += divisor
    return new_v


class LayerNorm2d(nn.LayerNorm):
    """LayerNorm over the channels of an NCHW map"""

    def forward(self, x):
        x = x.permute(0, 2, 3, 1)
        x = F.layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps)
        return x.permute(0, 3, 1, 2)


class SEModule(nn.Module):
    def __init__(self, channels, rd_ratio=0.25, bias=False):
        super().__init__()
        rd = make_divisible(channels * rd_ratio, 8, round_limit=0.)
        self.fc1 = nn.Conv2d(channels, rd, 1, bias=bias)
        self.bn = nn.Identity()
        self.act = nn.GELU()
        self.fc2 = nn.Conv2d(rd, channels, 1, bias=bias)
        self.gate = nn.Sigmoid()

    def forward(self, x):
        s = x.mean((2, 3), keepdim=True)
        return x * self.gate(self.fc2(self.act(self.bn(self.fc1(s)))))


class MbConvBlock(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv_dw = nn.Conv2d(c, c, 3, 1, 1, groups=c, bias=False)
        self.act = nn.GELU()
        self.se = SEModule(c)
        self.conv_pw = nn.Conv2d(c, c, 1, 1, 0, bias=False)

    def forward(self, x):
        return x + self.conv_pw(self.se(self.act(self.conv_dw(x))))


class Downsample2d(nn.Module):
    def __init__(self, dim, dim_out=None, norm_layer=LayerNorm2d):
        super().__init__()
        dim_out = dim_out or dim
        self.norm1 = norm_layer(dim)
        self.conv_block = MbConvBlock(dim)
        self.reduction = nn.Conv2d(dim, dim_out, 3, 2, 1, bias=False)
        self.norm2 = norm_layer(dim_out)

    def forward(self, x):
        return self.norm2(self.reduction(self.conv_block(self.norm1(x))))


class Stem(nn.Module):
    def __init__(self, in_chs, out_chs, norm_layer=LayerNorm2d):
        super().__init__()
        self.conv1 = nn.Conv2d(in_chs, out_chs, 3, 2, 1)
        self.down = Downsample2d(out_chs, norm_layer=norm_layer)

    def forward(self, x):
        return self.down(self.conv1(x))


class FeatureBlock(nn.Module):
    def __init__(self, dim, levels=0):
        super().__init__()
        reductions = levels
        self.blocks = nn.Sequential()
        for i in range(max(1, levels)):
            self.blocks.add_module(f'conv{i + 1}', MbConvBlock(dim))
            if reductions:
                self.blocks.add_module(f'pool{i + 1}', nn.MaxPool2d(3, 2, 1))
                reductions -= 1

    def forward(self, x):
        return self.blocks(x)


def gen_relative_position_index(window_size):
    """Swin's index, no class token: int64 [N][N]"""
    wh, ww = window_size
    coords = torch.stack(torch.meshgrid([torch.arange(wh), torch.arange(ww)], indexing='ij')).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += wh - 1
    rel[:, :, 1] += ww - 1
    rel[:, :, 0] *= 2 * ww - 1
    return rel.sum(-1)


class RelPosBias(nn.Module):
    def __init__(self, window_size, num_heads):
        super().__init__()
        self.window_size = window_size
        n = window_size[0] * window_size[1]
        self.bias_shape = (n, n, num_heads)
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window_size[0] - 1) * (2 * window_size[1] - 1), num_heads))
        self.register_buffer('relative_position_index', gen_relative_position_index(window_size), persistent=False)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)

    def get_bias(self):
        b = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(self.bias_shape)
        return b.permute(2, 0, 1).unsqueeze(0).contiguous()

    def forward(self, attn):
        return attn + self.get_bias()


class WindowAttentionGlobal(nn.Module):
    def __init__(self, dim, num_heads, window_size, use_global=True, qkv_bias=True):
        super().__init__()
        self.window_size = window_size
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.use_global = use_global
        self.rel_pos = RelPosBias(window_size=window_size, num_heads=num_heads)
        self.qkv = nn.Linear(dim, dim * (2 if use_global else 3), bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x, q_global=None):
        b, n, c = x.shape
        if self.use_global and q_global is not None:
            kv = self.qkv(x).reshape(b, n, 2, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4)
            k, v = kv.unbind(0)
            q = q_global.repeat(b // q_global.shape[0], 1, 1, 1)             # image-minor: window u <- image u mod B
            q = q.reshape(b, n, self.num_heads, self.head_dim).permute(0, 2, 1, 3)
        else:
            qkv = self.qkv(x).reshape(b, n, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4)
            q, k, v = qkv.unbind(0)
        attn = self.rel_pos((q * self.scale) @ k.transpose(-2, -1)).softmax(dim=-1)
        return self.proj((attn @ v).transpose(1, 2).reshape(b, n, c))


def window_partition(x, ws):
    b, h, w, c = x.shape
    x = x.view(b, h // ws[0], ws[0], w // ws[1], ws[1], c)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws[0], ws[1], c)


def window_reverse(windows, ws, img_size):
    h, w = img_size
    b = windows.shape[0] // (h * w // ws[0] // ws[1])
    x = windows.view(b, h // ws[0], w // ws[1], ws[0], ws[1], -1)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(b, h, w, -1)


class LayerScale(nn.Module):
    def __init__(self, dim, init_values=1e-5):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class GlobalContextVitBlock(nn.Module):
    def __init__(self, dim, num_heads, window_size, mlp_ratio=4., use_global=True, qkv_bias=True, layer_scale=None,
                 norm_layer=nn.LayerNorm):
        super().__init__()
        self.window_size = window_size
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttentionGlobal(dim, num_heads, window_size, use_global=use_global, qkv_bias=qkv_bias)
        self.ls1 = LayerScale(dim, layer_scale) if layer_scale is not None else nn.Identity()
        self.drop_path1 = nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))
        self.ls2 = LayerScale(dim, layer_scale) if layer_scale is not None else nn.Identity()
        self.drop_path2 = nn.Identity()

    def forward(self, x, q_global=None):
        b, h, w, c = x.shape
        win = window_partition(self.norm1(x), self.window_size).view(-1, self.window_size[0] * self.window_size[1], c)
        a = window_reverse(self.attn(win, q_global), self.window_size, (h, w))
        x = x + self.drop_path1(self.ls1(a))
        return x + self.drop_path2(self.ls2(self.mlp(self.norm2(x))))


class GlobalContextVitStage(nn.Module):
    def __init__(self, dim, depth, num_heads, feat_size, window_size, downsample=True, stage_norm=False, mlp_ratio=4.,
                 qkv_bias=True, layer_scale=None, norm_layer=LayerNorm2d, norm_layer_cl=nn.LayerNorm):
        super().__init__()
        if downsample:
            self.downsample = Downsample2d(dim, dim * 2, norm_layer=norm_layer)
            dim = dim * 2
            feat_size = (feat_size[0] // 2, feat_size[1] // 2)
        else:
            self.downsample = nn.Identity()
        self.feat_size = feat_size
        levels = int(math.log2(min(feat_size) / min(window_size)))
        self.global_block = FeatureBlock(dim, levels)
        self.global_norm = nn.Identity()
        self.blocks = nn.ModuleList([
            GlobalContextVitBlock(dim, num_heads, window_size, mlp_ratio=mlp_ratio, use_global=(i % 2 != 0), qkv_bias=qkv_bias,
                                  layer_scale=layer_scale, norm_layer=norm_layer_cl) for i in range(depth)])
        self.norm = norm_layer_cl(dim) if stage_norm else nn.Identity()
        self.dim = dim

    def forward(self, x):
        x = self.downsample(x)
        q_global = self.global_norm(self.global_block(x).permute(0, 2, 3, 1))
        x = x.permute(0, 2, 3, 1)
        for blk in self.blocks:
            x = blk(x, q_global)
        return self.norm(x).permute(0, 3, 1, 2).contiguous()


class GlobalContextVit(nn.Module):
    """the reference's backbone (no pooling, no classifier): NCHW [B, 8E, H/32, W/32]"""

    def __init__(self, in_channels=3, img_size=224, window_ratio=(32, 32, 16, 32), window_size=None, embed_dim=64,
                 depths=(3, 4, 19, 5), num_heads=(2, 4, 8, 16), mlp_ratio=3.0, qkv_bias=True, layer_scale=None, norm_eps=1e-5,
                 weight_init=''):
        super().__init__()
        n_st = len(depths)
        img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
        feat = tuple(d // 4 for d in img_size)
        if window_size is not None:
            window_size = tuple(window_size) if isinstance(window_size, (tuple, list)) else (window_size,) * n_st
            window_size = tuple((w, w) if isinstance(w, int) else tuple(w) for w in window_size)
        else:
            ratios = window_ratio if isinstance(window_ratio, (tuple, list)) else (window_ratio,) * n_st
            window_size = tuple((img_size[0] // r, img_size[1] // r) for r in ratios)
        n2d, ncl = partial(LayerNorm2d, eps=norm_eps), partial(nn.LayerNorm, eps=norm_eps)
        self.stem = Stem(in_channels, embed_dim, norm_layer=n2d)
        stages = []
        for i in range(n_st):
            sc = 2 ** max(i - 1, 0)
            stages.append(GlobalContextVitStage(embed_dim * sc, depths[i], num_heads[i], (feat[0] // sc, feat[1] // sc),
                                                window_size[i], downsample=i != 0, stage_norm=i == n_st - 1, mlp_ratio=mlp_ratio,
                                                qkv_bias=qkv_bias, layer_scale=layer_scale, norm_layer=n2d, norm_layer_cl=ncl))
        self.stages = nn.Sequential(*stages)
        for name, m in self.named_modules():
            if isinstance(m, nn.Linear):
                if weight_init == 'vit':
                    nn.init.xavier_uniform_(m.weight)
                    if m.bias is not None:
                        nn.init.normal_(m.bias, std=1e-6) if 'mlp' in name else nn.init.zeros_(m.bias)
                else:
                    nn.init.normal_(m.weight, std=.02)
                    if m.bias is not None:
                        nn.init.zeros_(m.bias)

    def forward_features(self, x):
        feats = [x]
        x = self.stem(x)
        for st in self.stages:
            x = st(x)
            feats.append(x)
        return feats

    def forward(self, x):
        return self.stages(self.stem(x))


VARIANTS = {
    'gcvit_xxtiny': dict(depths=(2, 2, 6, 2), num_heads=(2, 4, 8, 16)),
    'gcvit_xtiny': dict(depths=(3, 4, 6, 5), num_heads=(2, 4, 8, 16)),
    'gcvit_tiny': dict(depths=(3, 4, 19, 5), num_heads=(2, 4, 8, 16)),
    'gcvit_small': dict(depths=(3, 4, 19, 5), num_heads=(3, 6, 12, 24), embed_dim=96, mlp_ratio=2, layer_scale=1e-5),
    'gcvit_base': dict(depths=(3, 4, 19, 5), num_heads=(4, 8, 16, 32), embed_dim=128, mlp_ratio=2, layer_scale=1e-5),
}
BACKBONE_PARAMS = {'gcvit_xxtiny': 11482428, 'gcvit_xtiny': 19468294, 'gcvit_tiny': 27708974, 'gcvit_small': 50323173,
                   'gcvit_base': 89295836}
# the model of tests/test_gcvit_gpu.py: windows 7 / 7 / 14 / 7, a local and a global block in every stage
SMALL = dict(img_size=224, embed_dim=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8))
# the model of the CPU wiring test: 64 px, maps 16 / 8 / 4 / 2 with windows 4 / 4 / 4 / 2 (levels 2, 1, 0, 0)
TINY = dict(img_size=64, window_ratio=(16, 16, 16, 32), embed_dim=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8))


class Classifier(nn.Module):
    """backbone -> global average pool -> Linear: what ClassificationTask builds around a backbone"""

    def __init__(self, num_classes=10, **kw):
        super().__init__()
        self.backbone = GlobalContextVit(**kw)
        width = self.backbone.stages[-1].dim
        self.head = nn.Module()
        self.head.fc = nn.Linear(width, num_classes)

    def forward(self, x):
        return self.head.fc(self.backbone(x).mean((2, 3)))


def ref_state(ref, seed):
    """Every parameter non-trivial: norm gains off 1, biases off 0, tables and gammas off their init."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if n.endswith('.gamma'):
                p.copy_(0.5 + 0.2 * torch.randn(p.shape, generator=g))
            elif n.endswith('relative_position_bias_table'):
                p.copy_(torch.randn(p.shape, generator=g))
            elif p.dim() == 1 and n.endswith('.weight'):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1:
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / p[0].numel()) ** 0.5)
    return ref


# ---- the attention unit of the kernel contract -------------------------------------------------------------------------------
def window_index(b, h, w, ws):
    """int64 [b * nW][N]: the token row of token t of window u (u image-major: img * nW + wy * nWx + wx)"""
    idx = torch.arange(b * h * w).view(b, h // ws, ws, w // ws, ws)
    return idx.permute(0, 1, 3, 2, 4).reshape(-1, ws * ws)


def query_image(u, b, variant=None, nw=1):
    """the image whose q_global window u reads: u mod B (the reference's `repeat`); variant 'div': the wrong u div nW"""
    return u // nw if variant == 'div' else u % b


def _split(xw, parts, heads):
    bw, n, _ = xw.shape
    return xw.reshape(bw, n, parts, heads, HD).permute(2, 0, 3, 1, 4)


def _qkv(x, qg, geo, variant=None):
    """token rows (and q_global rows) -> q, k, v [Bw][heads][N][32]"""
    b, h, w, heads, ws = geo
    idx = window_index(b, h, w, ws)
    n, nw = ws * ws, (h // ws) * (w // ws)
    xw = x[idx]
    if qg is None:
        q, k, v = _split(xw, 3, heads)
    else:
        k, v = _split(xw, 2, heads)
        img = torch.tensor([query_image(u, b, variant, nw) for u in range(b * nw)])
        q = qg.view(b, n, heads, HD)[img].permute(0, 2, 1, 3)
    return q, k, v, idx


def _rows(t, idx, total):
    """[Bw][heads][N][32] -> token rows [total][heads*32]"""
    bw, heads, n, _ = t.shape
    out = torch.zeros(total, heads * HD, dtype=t.dtype)
    out[idx.reshape(-1)] = t.transpose(1, 2).reshape(bw * n, heads * HD)
    return out


def attention(qkv, qg, bias, geo):
    """the reference's softmax((q * scale) k^T + bias) v on token rows, any dtype -> rows [B*H*W][heads*32]"""
    b, h, w, heads, ws = geo
    q, k, v, idx = _qkv(qkv, qg, geo)
    p = ((q * SCALE) @ k.transpose(-2, -1) + bias.unsqueeze(0)).softmax(-1)
    return _rows(p @ v, idx, b * h * w)


class AttnRef:
    """fp64 forward / backward of bf16 qkv / q_global / dout and an fp32 bias, with the magnitude terms of every bound.
    grad: token rows of dq (None in global mode), dk, dv; dqg / m_dqg: rows [B*N][C] of d(q_global) in global mode."""

    def __init__(self, qkv, qg, bias, geo, dout):
        b, h, w, heads, ws = geo
        c, total, n = heads * HD, b * h * w, ws * ws
        nw = (h // ws) * (w // ws)
        x = qkv.double().requires_grad_(True)
        g = None if qg is None else qg.double().requires_grad_(True)
        bs = bias.double().requires_grad_(True)
        q, k, v, idx = _qkv(x, g, geo)
        s = (q @ k.transpose(-2, -1)) * SCALE + bs.unsqueeze(0)
        p = s.softmax(-1)
        o = p @ v
        _rows(o, idx, total).backward(dout.double())
        with torch.no_grad():
            go = _split(dout.double()[idx], 1, heads)[0]
            self.out = _rows(o.detach(), idx, total)
            self.lse = torch.logsumexp(s.detach(), -1)                      # [Bw][heads][N]
            pd, qa, ka, va, ga = p.detach(), q.detach().abs(), k.detach().abs(), v.detach().abs(), go.abs()
            self.m_out = _rows(pd @ va, idx, total)
            m_ds = pd * (ga @ va.transpose(-2, -1) + (ga * o.detach().abs()).sum(-1, keepdim=True))
            m_dq = SCALE * m_ds @ ka
            m_k, m_v = _rows(SCALE * m_ds.transpose(-2, -1) @ qa, idx, total), _rows(pd.transpose(-2, -1) @ ga, idx, total)
            if qg is None:
                self.grad = [x.grad[:, i * c:(i + 1) * c] for i in range(3)]
                self.m_grad = [_rows(m_dq, idx, total), m_k, m_v]
                self.dqg = self.m_dqg = None
            else:
                self.grad = [None, x.grad[:, :c], x.grad[:, c:2 * c]]
                self.m_grad = [None, m_k, m_v]
                self.dqg = g.grad
                img = torch.tensor([query_image(u, b) for u in range(b * nw)])
                m = torch.zeros(b, heads, n, HD, dtype=torch.float64).index_add_(0, img, m_dq)
                self.m_dqg = m.transpose(1, 2).reshape(b * n, c)
            self.dbias = bs.grad                      # [heads][N][N]
            self.m_dbias = m_ds.sum(0)


def emulate_kernel(qkv, qg, bias, geo, dout, variant=None):
    """The kernel's arithmetic in fp32 with its bf16 roundings: P rounded to bf16 before P V and before dV, delta formed as
    rowsum(P o dP) in fp32, dS rounded to bf16 before dQ / dK (d(bias) sums the unrounded dS), d(q_global) summed over its
    windows in fp32 and rounded once.  -> out bf16 rows, lse, d(qkv) bf16 rows, d(q_global) bf16 rows or None, dbias fp32.
    variant: None | 'div' (u div nW for u mod B) | 'no_scale' (the 32^-0.5 dropped)."""
    BF = torch.bfloat16
    b, h, w, heads, ws = geo
    total, n = b * h * w, ws * ws
    nw = (h // ws) * (w // ws)
    scale = 1.0 if variant == 'no_scale' else SCALE
    q, k, v, idx = _qkv(qkv.float(), None if qg is None else qg.float(), geo, variant)
    go = _split(dout.float()[idx], 1, heads)[0]
    s = (q @ k.transpose(-2, -1)) * scale + bias.float().unsqueeze(0)
    lse = torch.logsumexp(s, -1)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    o = ((e.to(BF).float() @ v) / e.sum(-1, keepdim=True)).to(BF)
    p = torch.exp(s - lse.unsqueeze(-1))
    dp = go @ v.transpose(-2, -1)
    delta = (p * dp).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    dv = p.to(BF).float().transpose(-2, -1) @ go
    dsb = ds.to(BF).float()
    dq, dk = (dsb @ k) * scale, (dsb.transpose(-2, -1) @ q) * scale
    out = _rows(o.float(), idx, total).to(BF)
    if qg is None:
        return out, lse, torch.cat([_rows(t, idx, total) for t in (dq, dk, dv)], 1).to(BF), None, ds.sum(0)
    img = torch.tensor([query_image(u, b, variant, nw) for u in range(b * nw)])
    dqg = torch.zeros(b, heads, n, HD).index_add_(0, img, dq).transpose(1, 2).reshape(b * n, heads * HD).to(BF)
    return out, lse, torch.cat([_rows(t, idx, total) for t in (dk, dv)], 1).to(BF), dqg, ds.sum(0)


def check_attention(ref, out, lse, dqkv, dqg, dbias, heads, scale=1.0, record=None):
    """The bounds of the GPU contract test (tests/test_gc_attn_contract_gpu.py), each multiplied by `scale` (the CPU test of the
    emulation asks for 0.7 of every bound).  They are those of tests/beit_ref.check_attention, whose derivation holds here
    unchanged (the reduction over the head dimension is 32 long instead of 64, which only shortens the fp32 sums):
    out element-wise |err| <= 2^-8 |ref| + 2^-7 (P |V|): one bf16 rounding of the result, one of P before P V, doubled;
    lse within 1e-3; gradients by token row against max(|ref row|, |magnitude row| / 4, 2^-24 of the largest magnitude row) at
    2e-2 — d(q_global) with the magnitudes of its windows added up, since its fp32 sum is rounded once;
    dbias element-wise |err| <= 2^-7 M + 2^-24 max M, M = sum over the windows of P (|dO| |V|^T + sum_d |dO| |O|).
    -> {name: worst error / bound}; raises AssertionError past 1."""
    c = heads * HD
    worst = {}
    err = (out.double() - ref.out).abs()
    worst['out'] = _ratio(err, (2.0 ** -8 * ref.out.abs() + 2.0 ** -7 * ref.m_out) * scale)
    worst['out_l2'] = float((out.double() - ref.out).norm() / ref.out.norm().clamp_min(1e-300)) / (1e-2 * scale)
    worst['lse'] = float((lse.double().reshape(ref.lse.shape) - ref.lse).abs().max()) / (1e-3 * scale)

    def rows(mine, want, mag):
        den = torch.maximum(torch.maximum(want.norm(dim=1), mag.norm(dim=1) / 4), mag.norm(dim=1).max() * 2.0 ** -24)
        return _ratio((mine.double() - want).norm(dim=1), den * 2e-2 * scale)
    names = ('dq', 'dk', 'dv') if ref.dqg is None else ('dk', 'dv')
    for i, what in enumerate(names):
        j = i if ref.dqg is None else i + 1
        worst[what] = rows(dqkv[:, i * c:(i + 1) * c], ref.grad[j], ref.m_grad[j])
    if ref.dqg is not None:
        worst['dq_global'] = rows(dqg, ref.dqg, ref.m_dqg)
    if dbias is not None:
        m = ref.m_dbias
        worst['dbias'] = _ratio((dbias.double() - ref.dbias).abs(), (2.0 ** -7 * m + 2.0 ** -24 * m.max()) * scale)
    if record is not None:
        record(worst)
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, f'error / bound (scale {scale}): {bad}'
    return worst


def _ratio(err, bound):
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float('inf'), 0.0))
    return float(torch.nan_to_num(r, nan=float('inf')).max()) if r.numel() else 0.0


def attn_inputs(geo, global_mode, seed):
    """bf16 qkv / q_global / dout rows and an fp32 bias N(0, 2^2) that moves the softmax"""
    b, h, w, heads, ws = geo
    c, n = heads * HD, ws * ws
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(b * h * w, (2 if global_mode else 3) * c, generator=g) * 1.5).to(torch.bfloat16)
    qg = (torch.randn(b * n, c, generator=g) * 1.5).to(torch.bfloat16) if global_mode else None
    dout = torch.randn(b * h * w, c, generator=g).to(torch.bfloat16)
    bias = torch.randn(heads, n, n, generator=g) * 2
    return qkv, qg, dout, bias


# ---- squeeze-excite with GELU inside and no biases ------------------------------------------------------------------------------
def se_ref(x, w1, w2, b1=None, b2=None, act='gelu', dout=None):
    """fp64: x [n][hw][c] -> out, (dx, dw1, dw2, db1, db2) when dout is given"""
    xd = x.double().requires_grad_(True)
    prm = [None if p is None else p.double().requires_grad_(True) for p in (w1, w2, b1, b2)]
    W1, W2, B1, B2 = prm
    m = xd.mean(1)
    pre = m @ W1.t() + (0 if B1 is None else B1)
    hid = F.gelu(pre) if act == 'gelu' else pre.relu()
    gate = torch.sigmoid(hid @ W2.t() + (0 if B2 is None else B2))
    out = xd * gate[:, None, :]
    if dout is None:
        return out.detach(), gate.detach()
    out.backward(dout.double())
    return out.detach(), gate.detach(), xd.grad, [None if p is None else p.grad for p in prm]
