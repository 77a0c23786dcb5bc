"""The restatement the BEiT tests measure against (tests/beit_ref.py), checked on its own: the relative-position index against
hand-written matrices, its attention against torch's scaled_dot_product_attention in fp64, an fp32 emulation of the kernel's
arithmetic inside half of every bound of the GPU contract test, and three wrong variants that each break a bound."""
import pytest
import torch
import torch.nn.functional as F

import beit_ref as R

BF = torch.bfloat16


def test_index_1x1():
    # T = 4: one patch-to-patch distance (0), cls -> token 1, token -> cls 2, cls -> cls 3
    assert R.gen_relative_position_index((1, 1)).tolist() == [[3, 1], [2, 0]]


def test_index_2x2():
    # T = 12; patch (r, c) -> 3 (r_i - r_j + 1) + (c_i - c_j + 1) over the raster order (0,0) (0,1) (1,0) (1,1)
    want = [[11, 9, 9, 9, 9],
            [10, 4, 3, 1, 0],
            [10, 5, 4, 2, 1],
            [10, 7, 6, 4, 3],
            [10, 8, 7, 5, 4]]
    assert R.gen_relative_position_index((2, 2)).tolist() == want


def test_index_3x2():
    # T = 18; 3 (r_i - r_j + 2) + (c_i - c_j + 1) over (0,0) (0,1) (1,0) (1,1) (2,0) (2,1)
    want = [[17, 15, 15, 15, 15, 15, 15],
            [16, 7, 6, 4, 3, 1, 0],
            [16, 8, 7, 5, 4, 2, 1],
            [16, 10, 9, 7, 6, 4, 3],
            [16, 11, 10, 8, 7, 5, 4],
            [16, 13, 12, 10, 9, 7, 6],
            [16, 14, 13, 11, 10, 8, 7]]
    idx = R.gen_relative_position_index((3, 2))
    assert idx.dtype == torch.int64 and idx.tolist() == want


def test_model_index_is_the_restated_one():
    from torchok_amd.models.backbones.beit import gen_relative_position_index
    for grid in ((1, 1), (2, 2), (3, 2), (14, 14), (7, 3)):
        assert torch.equal(gen_relative_position_index(grid), R.gen_relative_position_index(grid))


def _inputs(b, n, heads, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(b * n, 3 * heads * R.HD, generator=g) * 1.5).to(BF)
    dout = torch.randn(b * n, heads * R.HD, generator=g).to(BF)
    bias = torch.randn(heads, n, n, generator=g) * 2
    return qkv, dout, bias


def test_attention_equals_sdpa_in_fp64():
    b, n, heads = 2, 37, 3
    qkv, _, bias = _inputs(b, n, heads, 0)
    q, k, v = R.split_qkv(qkv.double(), b, n, heads)
    want = F.scaled_dot_product_attention(q, k, v, attn_mask=bias.double().unsqueeze(0)).transpose(1, 2).reshape(b * n, -1)
    got = R.attention(qkv.double(), bias.double(), b, n, heads)
    assert (got - want).abs().max() < 1e-12
    ref = R.AttnRef(qkv, bias, b, n, heads, torch.zeros(b * n, heads * R.HD))
    assert (ref.out - want).abs().max() < 1e-12


CASES = [(3, 5, 2), (2, 65, 2), (2, 197, 2)]


@pytest.mark.parametrize('b,n,heads', CASES)
def test_emulated_kernel_arithmetic_keeps_half_of_every_bound(b, n, heads):
    qkv, dout, bias = _inputs(b, n, heads, n)
    ref = R.AttnRef(qkv, bias, b, n, heads, dout)
    worst = R.check_attention(ref, *R.emulate_kernel(qkv, bias, b, n, heads, dout), heads, scale=0.5)
    assert set(worst) == {'out', 'out_l2', 'lse', 'dq', 'dk', 'dv', 'dbias'}


def test_bias_before_the_scale_breaks_a_bound():
    b, n, heads = 2, 65, 2
    qkv, dout, bias = _inputs(b, n, heads, 1)
    ref = R.AttnRef(qkv, bias, b, n, heads, dout)
    with pytest.raises(AssertionError):
        R.check_attention(ref, *R.emulate_kernel(qkv, bias, b, n, heads, dout, variant='bias_before_scale'), heads)


def test_transposed_index_breaks_a_bound():
    grid, heads, b = (3, 2), 2, 2
    n = grid[0] * grid[1] + 1
    g = torch.Generator().manual_seed(2)
    index = R.gen_relative_position_index(grid)
    table = torch.randn(int(index.max()) + 1, heads, generator=g) * 2
    qkv, dout, _ = _inputs(b, n, heads, 2)
    ref = R.AttnRef(qkv, R.relpos_bias(table, index), b, n, heads, dout)
    R.check_attention(ref, *R.emulate_kernel(qkv, R.relpos_bias(table, index), b, n, heads, dout), heads)
    with pytest.raises(AssertionError):
        R.check_attention(ref, *R.emulate_kernel(qkv, R.relpos_bias(table, index.t().contiguous()), b, n, heads, dout), heads)


def test_dbias_without_delta_breaks_its_bound():
    b, n, heads = 2, 65, 2
    qkv, dout, bias = _inputs(b, n, heads, 3)
    ref = R.AttnRef(qkv, bias, b, n, heads, dout)
    out, lse, dqkv, dbias = R.emulate_kernel(qkv, bias, b, n, heads, dout, variant='no_delta')
    good = R.emulate_kernel(qkv, bias, b, n, heads, dout)
    with pytest.raises(AssertionError, match='dbias'):
        R.check_attention(ref, good[0], good[1], good[2], dbias, heads)
