"""The plain-torch restatement of timm 0.6.13 gcvit (tests/gcvit_ref.py) against what is known of the original, and the bounds of
the attention contract against the fp32 emulation of the kernel's roundings.  CPU only."""
import pytest
import torch

import gcvit_ref as R


@pytest.mark.parametrize('name', sorted(R.VARIANTS))
def test_backbone_parameter_counts(name):
    """with 512 * embed_dim / 64 * 1000 + 1000 head parameters these are timm's published 12.00 / 19.98 / 28.22 / 51.09 / 90.32 M"""
    with torch.device('meta'):
        m = R.GlobalContextVit(**R.VARIANTS[name])
    n = sum(p.numel() for p in m.parameters())
    assert n == R.BACKBONE_PARAMS[name]
    width = 512 * R.VARIANTS[name].get('embed_dim', 64) // 64
    published = {'gcvit_xxtiny': 12.00, 'gcvit_xtiny': 19.98, 'gcvit_tiny': 28.22, 'gcvit_small': 51.09, 'gcvit_base': 90.32}
    assert round((n + width * 1000 + 1000) / 1e6, 2) == published[name]


def test_output_shape_and_key_names():
    m = R.GlobalContextVit(**R.VARIANTS['gcvit_xxtiny']).eval()
    with torch.no_grad():
        feats = m.forward_features(torch.randn(2, 3, 224, 224))
    assert [tuple(f.shape) for f in feats] == [(2, 3, 224, 224), (2, 64, 56, 56), (2, 128, 28, 28), (2, 256, 14, 14), (2, 512, 7, 7)]
    sd = m.state_dict()
    shapes = {
        'stem.conv1.weight': (64, 3, 3, 3), 'stem.conv1.bias': (64,), 'stem.down.norm1.weight': (64,),
        'stem.down.conv_block.conv_dw.weight': (64, 1, 3, 3), 'stem.down.conv_block.se.fc1.weight': (16, 64, 1, 1),
        'stem.down.conv_block.se.fc2.weight': (64, 16, 1, 1), 'stem.down.conv_block.conv_pw.weight': (64, 64, 1, 1),
        'stem.down.reduction.weight': (64, 64, 3, 3), 'stem.down.norm2.bias': (64,),
        'stages.0.global_block.blocks.conv3.conv_dw.weight': (64, 1, 3, 3),
        'stages.0.blocks.0.attn.qkv.weight': (192, 64), 'stages.0.blocks.1.attn.qkv.weight': (128, 64),      # k and v only
        'stages.0.blocks.1.attn.qkv.bias': (128,), 'stages.0.blocks.0.attn.proj.weight': (64, 64),
        'stages.0.blocks.0.attn.rel_pos.relative_position_bias_table': (169, 2),
        'stages.2.blocks.0.attn.rel_pos.relative_position_bias_table': (729, 8),
        'stages.0.blocks.0.mlp.fc1.weight': (192, 64), 'stages.0.blocks.0.mlp.fc2.bias': (64,),
        'stages.1.downsample.reduction.weight': (128, 64, 3, 3), 'stages.1.downsample.norm2.weight': (128,),
        'stages.1.global_block.blocks.conv2.se.fc1.weight': (32, 128, 1, 1),
        'stages.2.global_block.blocks.conv1.conv_pw.weight': (256, 256, 1, 1),
        'stages.3.norm.weight': (512,), 'stages.3.blocks.1.norm2.bias': (512,),
    }
    for k, s in shapes.items():
        assert k in sd and tuple(sd[k].shape) == s, k
    assert not any('relative_position_index' in k or 'global_norm' in k or '.ls1.' in k or '.bias' in k and '.se.' in k for k in sd)
    assert 'stages.0.global_block.blocks.conv4.conv_dw.weight' not in sd and 'stages.2.global_block.blocks.conv2.conv_dw.weight' not in sd
    assert 'stages.0.norm.weight' not in sd and 'stages.0.downsample.norm1.weight' not in sd
    small = R.GlobalContextVit(**R.VARIANTS['gcvit_small'])
    assert tuple(small.state_dict()['stages.0.blocks.0.ls1.gamma'].shape) == (96,)
    assert tuple(small.state_dict()['stem.down.conv_block.se.fc1.weight'].shape) == (24, 96, 1, 1)


def test_window_u_takes_the_query_of_image_u_mod_b():
    """B = 3 images of nW = 4 windows: perturbing q_global[1] changes exactly the windows 1, 4, 7, 10 (u mod B == 1), which lie
    in images 0, 1, 1, 2 — not the windows 4 ... 7 of image 1"""
    torch.manual_seed(0)
    attn = R.WindowAttentionGlobal(32, 1, (2, 2), use_global=True).eval()
    x = torch.randn(12, 4, 32)
    qg = torch.randn(3, 2, 2, 32)
    with torch.no_grad():
        base = attn(x, qg)
        other = qg.clone()
        other[1] += 1.0
        moved = attn(x, other)
    changed = [u for u in range(12) if not torch.equal(base[u], moved[u])]
    assert changed == [1, 4, 7, 10]
    # the contract's reference says the same
    geo = (3, 4, 4, 1, 2)
    qkv, qgr, dout, bias = R.attn_inputs(geo, True, 3)
    idx = R.window_index(*geo[:3], geo[4])
    a = R.attention(qkv.double(), qgr.double(), bias.double(), geo)
    qgr2 = qgr.clone()
    qgr2[4:8] = (qgr2[4:8].float() + 1).to(qgr2.dtype)
    b = R.attention(qkv.double(), qgr2.double(), bias.double(), geo)
    assert [u for u in range(12) if not torch.equal(a[idx[u]], b[idx[u]])] == [1, 4, 7, 10]


def test_contract_reference_is_the_module():
    """gcvit_ref.attention on token rows is WindowAttentionGlobal between qkv and proj (partition and reverse included)"""
    torch.manual_seed(1)
    b, h, w, heads, ws = 3, 4, 6, 2, 2
    c = heads * 32
    for use_global in (False, True):
        attn = R.WindowAttentionGlobal(c, heads, (ws, ws), use_global=use_global).double().eval()
        with torch.no_grad():
            attn.rel_pos.relative_position_bias_table.normal_()
        parts = 2 if use_global else 3
        qkv = torch.randn(b * h * w, parts * c, dtype=torch.float64)
        qg = torch.randn(b, ws, ws, c, dtype=torch.float64) if use_global else None
        captured = {}
        attn.qkv = _Give(qkv, b, h, w, ws)
        attn.proj = _Take(captured)
        with torch.no_grad():
            attn(torch.zeros((b * (h // ws) * (w // ws), ws * ws, c), dtype=torch.float64), qg)
            bias = attn.rel_pos.get_bias()[0]
            mine = R.attention(qkv, None if qg is None else qg.reshape(b * ws * ws, c), bias, (b, h, w, heads, ws))
        want = R.window_reverse(captured['x'].view(-1, ws, ws, c), (ws, ws), (h, w)).reshape(b * h * w, c)
        assert torch.allclose(mine, want, rtol=1e-12, atol=1e-12)


class _Give(torch.nn.Module):
    """stands in for attn.qkv: returns the window-partitioned rows of a given qkv matrix"""

    def __init__(self, rows, b, h, w, ws):
        super().__init__()
        self.win = R.window_partition(rows.view(b, h, w, -1), (ws, ws)).view(-1, ws * ws, rows.shape[1])

    def forward(self, x):
        return self.win


class _Take(torch.nn.Module):
    def __init__(self, box):
        super().__init__()
        self.box = box

    def forward(self, x):
        self.box['x'] = x
        return x


CASES = [(3, 14, 21, 2, 7), (2, 28, 14, 1, 14), (1, 8, 8, 3, 8), (2, 8, 4, 1, 4)]


@pytest.mark.parametrize('global_mode', [False, True], ids=['local', 'global'])
@pytest.mark.parametrize('geo', CASES, ids=lambda g: 'b%d_%dx%d_h%d_ws%d' % g)
def test_the_emulated_kernel_meets_the_bounds_with_margin(geo, global_mode):
    """The bounds leave room beyond the kernel's own roundings.  For `out` the room is known: one bf16 rounding of the result
    (2^-8 |ref|) and one of P before P V (2^-8 P |V|) against 2^-8 |ref| + 2^-7 P |V| with P |V| >= |ref| is at most 2 / 3 of
    the bound, so 0.7 is asked of everything (the gradients and lse sit far below it)."""
    qkv, qg, dout, bias = R.attn_inputs(geo, global_mode, seed=11)
    ref = R.AttnRef(qkv, qg, bias, geo, dout)
    R.check_attention(ref, *R.emulate_kernel(qkv, qg, bias, geo, dout), geo[3], scale=0.7)


@pytest.mark.parametrize('variant', ['div', 'no_scale'])
def test_the_bounds_catch_the_wrong_forms(variant):
    geo = CASES[0]
    qkv, qg, dout, bias = R.attn_inputs(geo, True, seed=12)
    ref = R.AttnRef(qkv, qg, bias, geo, dout)
    with pytest.raises(AssertionError):
        R.check_attention(ref, *R.emulate_kernel(qkv, qg, bias, geo, dout, variant=variant), geo[3])
