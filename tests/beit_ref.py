"""Plain-torch restatement of the reference BEiT (torchok/models/backbones/beit.py:61-203 on [timm 0.6.13] beit Attention / Block /
gen_relative_position_index): the oracle of tests/test_beit*.py, in fp32 and, after .double(), fp64.  Module names are timm's, so
state_dicts load both ways (the FPN containers of the reference are left out: they hold no part of forward()).  It lives under
tests/ because oracle/ is frozen and the reference imports timm.  The attention arithmetic of the contract tests (fp64 reference,
fp32 emulation of the kernel's roundings, the magnitudes of its bounds) is here too, so that the CPU and GPU tests share it."""
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

HD = 64


def gen_relative_position_index(window_size):
    wh, ww = window_size
    t = (2 * wh - 1) * (2 * ww - 1) + 3
    coords = torch.stack(torch.meshgrid([torch.arange(wh), torch.arange(ww)], indexing='ij')).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += wh - 1
    rel[:, :, 1] += ww - 1
    rel[:, :, 0] *= 2 * ww - 1
    index = torch.zeros((wh * ww + 1,) * 2, dtype=rel.dtype)
    index[1:, 1:] = rel.sum(-1)
    index[0, 0:] = t - 3
    index[0:, 0] = t - 2
    index[0, 0] = t - 1
    return index


def relpos_bias(table, index):
    """[heads][N][N] = table[index.view(-1)].view(N, N, heads).permute(2, 0, 1)"""
    n = index.shape[0]
    return table[index.reshape(-1)].view(n, n, -1).permute(2, 0, 1).contiguous()


class PatchEmbed(nn.Module):
    def __init__(self, img_size, patch_size, in_chans, embed_dim):
        super().__init__()
        self.img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
        self.grid_size = (self.img_size[0] // patch_size, self.img_size[1] // patch_size)
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.proj = nn.Conv2d(in_chans, embed_dim, patch_size, patch_size)

    def forward(self, x):
        return self.proj(x).flatten(2).transpose(1, 2)


class Attention(nn.Module):
    def __init__(self, dim, num_heads, qkv_bias, window_size):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=False)
        if qkv_bias:
            self.q_bias = nn.Parameter(torch.zeros(dim))
            self.register_buffer('k_bias', torch.zeros(dim), persistent=False)
            self.v_bias = nn.Parameter(torch.zeros(dim))
        else:
            self.q_bias = self.k_bias = self.v_bias = None
        if window_size:
            t = (2 * window_size[0] - 1) * (2 * window_size[1] - 1) + 3
            self.relative_position_bias_table = nn.Parameter(torch.zeros(t, num_heads))
            self.register_buffer('relative_position_index', gen_relative_position_index(window_size))
        else:
            self.relative_position_bias_table = self.relative_position_index = None
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, N, C = x.shape
        qkv_bias = torch.cat((self.q_bias, self.k_bias, self.v_bias)) if self.q_bias is not None else None
        qkv = F.linear(x, self.qkv.weight, qkv_bias).reshape(B, N, 3, self.num_heads, -1).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.unbind(0)
        attn = (q * self.scale) @ k.transpose(-2, -1)
        if self.relative_position_bias_table is not None:
            attn = attn + relpos_bias(self.relative_position_bias_table, self.relative_position_index).unsqueeze(0)
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
    def __init__(self, dim, num_heads, mlp_ratio, qkv_bias, norm_layer, init_values, window_size):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads, qkv_bias, window_size)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))
        if init_values:
            self.gamma_1 = nn.Parameter(init_values * torch.ones(dim))
            self.gamma_2 = nn.Parameter(init_values * torch.ones(dim))
        else:
            self.gamma_1 = self.gamma_2 = None
        self.drop_scales = None       # (scale1, scale2) per-sample vectors: stochastic depth with pinned draws

    def forward(self, x):
        s1, s2 = self.drop_scales or (None, None)
        a = self.attn(self.norm1(x))
        if self.gamma_1 is not None:
            a = self.gamma_1 * a
        x = x + (a if s1 is None else a * s1[:, None, None].to(a.dtype))
        m = self.mlp(self.norm2(x))
        if self.gamma_2 is not None:
            m = self.gamma_2 * m
        return x + (m if s2 is None else m * s2[:, None, None].to(m.dtype))


class Beit(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_channels=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.,
                 qkv_bias=True, norm_layer=None, init_values=None, use_abs_pos_emb=True, use_rel_pos_bias=False):
        super().__init__()
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        self.patch_embed = PatchEmbed(img_size, patch_size, in_channels, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches + 1, embed_dim)) if use_abs_pos_emb else None
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio, qkv_bias, norm_layer, init_values,
                                           self.patch_embed.grid_size if use_rel_pos_bias else None) for _ in range(depth)])
        self.norm = norm_layer(embed_dim)

    def forward(self, x):
        x = self.patch_embed(x)
        x = torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1)
        if self.pos_embed is not None:
            x = x + self.pos_embed
        for blk in self.blocks:
            x = blk(x)
        return self.norm(x)[:, 0][..., None, None]


class Classifier(nn.Module):
    """ClassificationTask(backbone, pooling=Pooling, head=ClassificationHead): backbone.* / head.fc.*."""

    def __init__(self, num_classes, **kwargs):
        super().__init__()
        self.backbone = Beit(**kwargs)
        self.head = nn.Module()
        self.head.fc = nn.Linear(self.backbone.norm.normalized_shape[0], num_classes)

    def forward(self, x):
        return self.head.fc(self.backbone(x).mean((2, 3)))


# ---- the attention unit of the kernel contract -------------------------------------------------------------------------------
def split_qkv(qkv, b, n, heads):
    """rows [b*n][3*heads*64] -> q, k, v [b][heads][n][64]"""
    return qkv.reshape(b, n, 3, heads, HD).permute(2, 0, 3, 1, 4)


def attention(qkv, bias, b, n, heads):
    """timm's softmax((q * scale) k^T + bias) v on token rows, any dtype -> rows [b*n][heads*64]"""
    q, k, v = split_qkv(qkv, b, n, heads)
    p = ((q * 0.125) @ k.transpose(-2, -1) + bias.unsqueeze(0)).softmax(-1)
    return (p @ v).transpose(1, 2).reshape(b * n, heads * HD)


class AttnRef:
    """fp64 forward / backward of bf16 qkv / dout and an fp32 bias, with the magnitude terms of every bound.
    variant: None, or one of the wrong forms the CPU test shows the bounds catch."""

    def __init__(self, qkv, bias, b, n, heads, dout):
        c = heads * HD
        x = qkv.double().requires_grad_(True)
        bs = bias.double().requires_grad_(True)
        q, k, v = split_qkv(x, b, n, heads)
        s = (q @ k.transpose(-2, -1)) * 0.125 + bs.unsqueeze(0)
        p = s.softmax(-1)
        o = p @ v
        o.transpose(1, 2).reshape(b * n, c).backward(dout.double())
        with torch.no_grad():
            go = dout.double().reshape(b, n, heads, HD).transpose(1, 2)
            self.out = o.detach().transpose(1, 2).reshape(b * n, c)
            self.lse = torch.logsumexp(s.detach(), -1)
            pd, qa, ka, va, ga = p.detach(), q.detach().abs(), k.detach().abs(), v.detach().abs(), go.abs()
            self.m_out = (pd @ va).transpose(1, 2).reshape(b * n, c)
            m_ds = pd * (ga @ va.transpose(-2, -1) + (ga * o.detach().abs()).sum(-1, keepdim=True))
            tok = lambda t: t.transpose(1, 2).reshape(b * n, c)        # noqa: E731
            self.m_grad = [tok(0.125 * m_ds @ ka), tok(0.125 * m_ds.transpose(-2, -1) @ qa), tok(pd.transpose(-2, -1) @ ga)]
            self.grad = [x.grad[:, i * c:(i + 1) * c] for i in range(3)]
            self.dbias = bs.grad                      # [heads][n][n]
            self.m_dbias = m_ds.sum(0)                # sum_b P (|dO| |V|^T + sum_d |dO| |O|)


def emulate_kernel(qkv, bias, b, n, heads, dout, variant=None):
    """The kernel's arithmetic in fp32 with its bf16 roundings: P rounded to bf16 before P V and before dV, O stored in bf16
    before delta = rowsum(dO o O), dS rounded to bf16 before dQ / dK (d(bias) sums the unrounded dS); results rounded to bf16.
    -> out bf16 rows, lse fp32, dqkv bf16 rows, dbias fp32.  variant: 'bias_before_scale' | 'no_delta' | None."""
    BF = torch.bfloat16
    c = heads * HD
    q, k, v = (t.float() for t in split_qkv(qkv, b, n, heads))
    go = dout.float().reshape(b, n, heads, HD).transpose(1, 2)
    bias = bias.float().unsqueeze(0)
    s = (q @ k.transpose(-2, -1) + bias) * 0.125 if variant == 'bias_before_scale' else (q @ k.transpose(-2, -1)) * 0.125 + bias
    lse = torch.logsumexp(s, -1)
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    o = ((e.to(BF).float() @ v) / e.sum(-1, keepdim=True)).to(BF)
    p = torch.exp(s - lse.unsqueeze(-1))
    delta = (go * o.float()).sum(-1, keepdim=True)
    if variant == 'no_delta':
        delta = torch.zeros_like(delta)
    ds = p * (go @ v.transpose(-2, -1) - delta)
    dv = p.to(BF).float().transpose(-2, -1) @ go
    dsb = ds.to(BF).float()
    dq, dk = (dsb @ k) * 0.125, (dsb.transpose(-2, -1) @ q) * 0.125
    tok = lambda t: t.transpose(1, 2).reshape(b * n, c)        # noqa: E731
    return tok(o.float()).to(BF), lse, torch.cat([tok(dq), tok(dk), tok(dv)], 1).to(BF), ds.sum(0)


def check_attention(ref, out, lse, dqkv, dbias, heads, scale=1.0, record=None):
    """The bounds of the GPU contract test (tests/test_beit_attn_contract_gpu.py), each multiplied by `scale` (the CPU test of
    the emulation asks for half of every bound).  -> {name: worst error / bound}; raises AssertionError past 1.
    out / dq / dk / dv: the bounds of tests/test_global_attn_contract_gpu.py (restated): out element-wise
    |err| <= 2^-8 |ref| + 2^-7 (P |V|); gradients by token row against max(|ref row|, |magnitude row| / 4, 2^-24 of the largest
    magnitude row) at 2e-2.  lse within 1e-3.  dbias element-wise |err| <= 2^-7 M + 2^-24 max M."""
    c = heads * HD
    worst = {}
    err = (out.double() - ref.out).abs()
    bound = 2.0 ** -8 * ref.out.abs() + 2.0 ** -7 * ref.m_out
    worst['out'] = _ratio(err, bound * scale)
    worst['out_l2'] = float((out.double() - ref.out).norm() / ref.out.norm().clamp_min(1e-300)) / (1e-2 * scale)
    worst['lse'] = float((lse.double().view(ref.lse.shape) - ref.lse).abs().max()) / (1e-3 * scale)
    for i, what in enumerate(('dq', 'dk', 'dv')):
        mine, want, mag = dqkv[:, i * c:(i + 1) * c].double(), ref.grad[i], ref.m_grad[i]
        den = torch.maximum(torch.maximum(want.norm(dim=1), mag.norm(dim=1) / 4), mag.norm(dim=1).max() * 2.0 ** -24)
        worst[what] = _ratio((mine - want).norm(dim=1), den * 2e-2 * scale)
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


# ---- shared by tests/test_beit.py and tests/test_beit_gpu.py -----------------------------------------------------------------
TINY = dict(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2, init_values=0.1, use_abs_pos_emb=False,
            use_rel_pos_bias=True)                                          # the restatement's arguments of the tiny model ...
TINY_BP = dict(img_size=64, embed_dim=128, depth=2, num_heads=2)            # ... and what beit_base_patch16_224 needs to be told


def ref_state(ref, seed):
    """Every parameter non-trivial: LayerNorm gains off 1, biases off 0, tables and gammas off their init."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if n.endswith(('norm1.weight', 'norm2.weight', 'norm.weight')):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
            elif 'gamma_' in n:
                p.copy_(0.5 + 0.2 * torch.randn(p.shape, generator=g))
            elif n.endswith('relative_position_bias_table'):
                p.copy_(torch.randn(p.shape, generator=g))
            elif p.dim() == 1 or n.endswith(('cls_token', 'pos_embed')):
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / p[0].numel()) ** 0.5)
    return ref


def beit_config(backbone='beit_base_patch16_224', num_classes=10, optimizer='SGD', opt_params=None, backbone_params=None, side=64):
    from torchok_amd.constructor.config import apply_schema
    cfg = {
        'task': {'name': 'ClassificationTask',
                 'params': {'backbone_name': backbone,
                            'backbone_params': dict({'in_channels': 3}, **(backbone_params or {})),
                            'pooling_name': 'Pooling', 'head_name': 'ClassificationHead',
                            'head_params': {'num_classes': num_classes},
                            'inputs': [{'shape': [3, side, side], 'dtype': 'float32'}]}},
        'joint_loss': {'losses': [{'name': 'CrossEntropyLoss', 'mapping': {'input': 'prediction', 'target': 'target'}}]},
        'optimization': [{'optimizer': {'name': optimizer,
                                        'params': opt_params or {'lr': 0.1, 'momentum': 0.9, 'weight_decay': 1e-4}}}],
        'data': {}, 'trainer': {'precision': 'bf16'},
    }
    return apply_schema(cfg)


def beit_task(**kw):
    import torchok_amd as T
    cfg = beit_config(**kw)
    return T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)


def copy_backbone_state(ref, model):
    """the restatement's state into a model that also owns the FPN containers"""
    sd, dsd = ref.state_dict(), model.state_dict()
    missing = [k for k in sd if k not in dsd]
    assert not missing, missing
    with torch.no_grad():
        for k, v in sd.items():
            dsd[k].copy_(v)
