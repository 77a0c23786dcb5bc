"""tests/mlp_rows_ref.py held to torch: every fp64 reference equals torch's own operation (F.gelu and its autograd derivative, an fp64
Mlp forward and backward through autograd, F.unfold-style expressions of patch merge and patch gather, the relative_position_index of
the SwinV2 oracle); an fp32 restatement (torch fp32 products, the kernel's rounding points, F.gelu) stays inside HALF of the
non-rounding part of every bound; the bounds reject wrong variants; the launcher's rules are restated consistently; and
tok_mlp_serves is pinned at its 2^32-byte boundary host-side (no launch, no buffer).

Measured here: torch's fp32 F.gelu rounded to bf16 reaches 0.97 of the GELU bound over all finite bf16 inputs below 1e38, all of it
from the final rounding; the numpy restatement of the polynomial of tok_common.h reaches 0.36 of the 2^-20 term for GELU and 0.37 for
GELU'; tanh-GELU reaches 31 x the bound (at x = -3.375) with 0.25 % of the bf16 inputs over it."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from helpers import A_BF, BF, U32
import mlp_rows_ref as M

F64 = torch.float64


def ratio(err, bound):
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float('inf'), 0.0))
    return float(torch.nan_to_num(r, nan=float('inf')).max())


def finite_table(limit=float('inf')):
    x = M.bf16_table()
    return x[torch.isfinite(x.float()) & (x.float().abs() <= limit)]


# ---- the references are torch's own operations ----------------------------------------------------------------------------------
def test_gelu_and_its_derivative_are_torchs():
    x = finite_table(1e4).double().requires_grad_(True)
    y = F.gelu(x)
    g, = torch.autograd.grad(y.sum(), x)
    assert float((M.gelu(x.detach()) - y.detach()).abs().max()) <= 1e-15 * 1e4
    assert float((M.gelu_d(x.detach()) - g).abs().max()) <= 1e-12
    xs = torch.tensor([-6.0, -5.6, -3.5, -1.0, -0.0, 0.0, 1.0, 5.6, 6.0], dtype=F64)
    assert torch.equal(M.act_d(0, xs), (xs > 0).double()) and torch.equal(M.act_d(2, xs), torch.ones_like(xs))


@pytest.mark.parametrize('c', M.WIDTHS)
def test_stage_references_chain_to_an_fp64_mlp(c):
    """without the stage-wise re-entry (every stage fed the fp64 result of the one before) the references are nn.Linear -> GELU ->
    nn.Linear and its autograd gradients"""
    d = M.make_mlp(c, 37, seed=c)
    fc1, fc2 = nn.Linear(c, 4 * c).double(), nn.Linear(4 * c, c).double()
    with torch.no_grad():
        fc1.weight.copy_(d['w1'].double())
        fc1.bias.copy_(d['b1'].double())
        fc2.weight.copy_(d['w2'].double())
        fc2.bias.copy_(d['b2'].double())
    x = d['x'].double().requires_grad_(True)
    pre = fc1(x)
    pre.retain_grad()
    y = fc2(F.gelu(pre))
    mine_pre, _ = M.pre_ref(d)
    mine_y, _ = M.y_ref(d, M.gelu(mine_pre))
    assert torch.allclose(mine_pre, pre.detach(), rtol=0, atol=1e-12) and torch.allclose(mine_y, y.detach(), rtol=0, atol=1e-12)
    # backward: the kernel is handed pre rows and dgrad packs; W2_dgrad [hidden][c] = W2^T, W1_dgrad [c][hidden] = W1^T
    e = dict(d, w2d=d['w2'].t().contiguous(), w1d=d['w1'].t().contiguous(), pre=pre.detach())
    y.backward(d['dy'].double())
    dpre, _, _ = M.dpre_ref(e)
    dx, _, _ = M.dx_ref(e, dpre, acc=False)
    assert torch.allclose(dpre, pre.grad, rtol=0, atol=1e-12) and torch.allclose(dx, x.grad, rtol=0, atol=1e-12)
    dxa, _, _ = M.dx_ref(e, dpre, acc=True)
    assert torch.equal(dxa, dx + d['prior'].double())


@pytest.mark.parametrize('rows,c,cls', M.MLP_CASES)
def test_forward_cases_reach_both_clamps_and_the_negative_tail(rows, c, cls):
    """asserted on fp64: every case has pre-activations below -5.6, above +5.6 and inside (-4, -3); the backward's pre rows too"""
    d = M.make_mlp(c, min(rows, M.P), seed=rows + c)
    assert M.reaches_the_tails(M.pre_ref(d)[0]) and M.reaches_the_tails(d['pre'])
    assert M.mlp_class(rows, c) == cls and (cls == 'wrap') == (M.mlp_tiles(rows, c) > M.GRID_CAP)


def test_launch_rules_restated():
    assert [M.mlp_tiles(r, c) for r, c, k in M.MLP_CASES if k == 'wrap'] == [258, 258, 258]
    assert M.mlp_tiles(70000, 96) == 274 and M.mlp_tiles(33000, 192) == 129 and M.mlp_tiles(16500, 384) == 129
    assert M.act_blocks(65536) == 32 and M.act_blocks(M.ACT_TRIP) == 65536 and M.act_blocks(M.ACT_TRIP + 2048) == 65536
    assert [M.cpb_class(ws) for ws in M.CPB_WS] == list(M.CPB_WS.values())


def serves_boundaries():
    for c in M.WIDTHS:
        h, t = 4 * c, M.TILE[c]
        top = (2 ** 32 - 1) // (h * 2)                    # the largest row count with rows * hidden * 2 < 2^32
        full = top // t * t                               # the largest whole-tile count below 2^32 bytes
        for rows in (full - t, full - 1, full, full + 1, full + t - 1, top - 1, top, top + 1, full + t, full + t + 1):
            yield rows, c, h


def test_mlp_serves_counts_the_whole_last_tile(fake_backend):
    """the kernels form 32-bit byte offsets (tok_row * H + ...) * 2 for EVERY row of the last tile and leave the rows past `rows` to
    the buffer range check; once such an offset wraps past 2^32 it is a small in-range one again and the SAVE stores (pre, act,
    dpre) would land in the first rows.  rows * hidden * 2 < 2^32 alone admitted such row counts (e.g. c = 384: 1398101 rows, the
    last tile ends 43 rows past 2^32 bytes); the rule is the tile-rounded count now.  Host-side only: no launch, no 4 GB buffer."""
    from torchok_amd import _C
    lib = _C.load_library()
    old_rule_admits_a_wrapping_case = False
    for rows, c, h in serves_boundaries():
        want = int(M.mlp_tiles(rows, c) * M.TILE[c] * h * 2 < 2 ** 32)
        assert M.mlp_serves(rows, c, h) == want
        assert lib.tok_mlp_serves(rows, c, h) == want, (rows, c)
        assert fake_backend.tok_mlp_serves(rows, c, h) == want, (rows, c)
        old_rule_admits_a_wrapping_case |= (rows * h * 2 < 2 ** 32 and not want)
    assert old_rule_admits_a_wrapping_case
    for c in M.WIDTHS:
        assert lib.tok_mlp_serves(0, c, 4 * c) == 0 and lib.tok_mlp_serves(1, c, 4 * c) == 1 and lib.tok_mlp_serves(1, c, 2 * c) == 0
    assert lib.tok_mlp_serves(1000, 768, 3072) == 0 and lib.tok_mlp_serves(1000, 100, 400) == 0


@pytest.mark.parametrize('ws', [4, 7])
def test_swin_index_is_the_oracles(ws):
    import oracle.swin_ref as S
    attn = S.WindowAttention(32, (ws, ws), 1)
    assert torch.equal(M.swin_index(ws), attn.relative_position_index)
    assert int(M.swin_index(ws).max()) == (2 * ws - 1) ** 2 - 1
    d = M.make_cpb(ws, 3, seed=ws)
    table = d['table'].double().requires_grad_(True)
    n = ws * ws
    bias = 16 * torch.sigmoid(table[attn.relative_position_index.view(-1)].view(n, n, -1).permute(2, 0, 1).contiguous())
    assert torch.allclose(M.cpb_fwd_ref(d['table'], d['index'])[0], bias.detach(), rtol=0, atol=1e-13)
    bias.backward(d['dbias'].double())
    assert torch.allclose(M.cpb_bwd_ref(d, 0)[0], table.grad, rtol=0, atol=1e-11)
    dt = dict(d, dbias=d['dbias'].transpose(1, 2).contiguous())           # stored [h][j][i]
    assert torch.allclose(M.cpb_bwd_ref(dt, 1)[0], table.grad, rtol=0, atol=1e-11)
    assert bool((table.grad[-M.CPB_SPARE_ROWS:] == 0).all())


@pytest.mark.parametrize('b,h,w,c', M.MERGE_CASES)
def test_patch_merge_is_an_unfold(b, h, w, c):
    x = torch.arange(b * h * w * c, dtype=F64).view(b, h, w, c)
    # F.unfold over 2x2 blocks, stride 2: channel-major (c, ky, kx); PatchMerging's order is (kx, ky, c)
    u = F.unfold(x.permute(0, 3, 1, 2), 2, stride=2).view(b, c, 2, 2, h // 2, w // 2)
    want = u.permute(0, 4, 5, 3, 2, 1).reshape(b, h // 2, w // 2, 4 * c)
    assert torch.equal(M.patch_merge_ref(x), want)
    assert not torch.equal(M.patch_merge_ref(x, (0, 2, 1, 3)), want)


@pytest.mark.parametrize('n,h,w,p', M.GATHER_CASES)
def test_patch_gather_is_an_unfold(n, h, w, p):
    img = torch.arange(n * h * w * 4, dtype=F64).view(n, h, w, 4)
    u = F.unfold(img.permute(0, 3, 1, 2), p, stride=p).view(n, 4, p, p, -1)          # (ch, py, px) x patches
    want = u.permute(0, 4, 2, 3, 1).reshape(n * (h // p) * (w // p), p * p * 4)
    assert torch.equal(M.patch_gather_ref(img, p), want)


# ---- an fp32 run stays inside half of the non-rounding part of every bound ----------------------------------------------------------
def test_fp32_gelu_against_the_bound_over_every_bf16_input():
    x = finite_table(1e38)
    ref, bound = M.act_fwd_ref(1, x)
    f32 = F.gelu(x.float())
    assert ratio((f32.double() - ref).abs(), 0.5 * M.gelu_slack(x)) <= 1.0                  # before the rounding
    r = ratio((f32.to(BF).double() - ref).abs(), bound)
    assert 0.9 < r <= 1.0, r                                                                 # measured: 0.97
    relu, zero = M.act_fwd_ref(0, x)
    assert torch.equal(relu, F.relu(x.double())) and not bool(zero.any())


def test_the_polynomial_restated_in_numpy_stays_inside_half_of_the_slack():
    x = finite_table()
    rf = ratio((M.gelu_poly(x).double() - M.gelu(x)).abs(), M.gelu_slack(x))
    rd = ratio((M.gelu_d_poly(x).double() - M.gelu_d(x)).abs(), M.gelu_slack(x))
    assert rf <= 0.5 and rd <= 0.5, (rf, rd)                                                 # measured: 0.36, 0.37


@pytest.mark.parametrize('kind', [0, 1, 2])
@pytest.mark.parametrize('acc', [0, 1])
def test_fp32_activation_backward_stays_inside_half_of_the_slack(kind, acc):
    x = finite_table(1e38)
    g, prev = M.make_act_bwd()
    keep = torch.isfinite(M.bf16_table().float()) & (M.bf16_table().float().abs() <= 1e38)
    g, prev = g[keep], (prev[keep] if acc else None)
    ref, bound = M.act_bwd_ref(kind, g, x, prev)
    xr = x.float().requires_grad_(True)
    d32 = (xr > 0).float() if kind == 0 else torch.autograd.grad(F.gelu(xr).sum(), xr)[0] if kind == 1 else torch.ones_like(xr)
    mine = g.float() * d32 + (prev.float() if acc else 0.0)
    assert ratio((mine.double() - ref).abs(), 0.5 * M.act_bwd_slack(kind, g, x, prev)) <= 1.0
    assert ratio((mine.to(BF).double() - ref).abs(), bound) <= 1.0
    # accumulate treated as overwrite is rejected
    if acc:
        wrong = (g.float() * d32).to(BF).double()
        assert ratio((wrong - ref).abs(), bound) > 1.0


@pytest.mark.parametrize('c', M.WIDTHS)
@pytest.mark.parametrize('acc', [0, 1])
def test_fp32_mlp_stays_inside_half_of_the_slack(c, acc):
    d = M.make_mlp(c, 77, seed=c + 1)
    f = M.mlp_fp32(d, acc)

    def inside(what, mine32, ref, bound, slack):
        assert ratio((mine32.double() - ref).abs(), 0.5 * slack) <= 1.0, what
        assert ratio((mine32.to(BF).double() - ref).abs(), bound) <= 1.0, what
    ref, bound = M.pre_ref(d)
    inside('pre', f['pre'], ref, bound, bound - A_BF * ref.abs())
    ref, bound = M.act_ref(f['pre_own'])
    inside('act', f['act'], ref, bound, M.gelu_slack(f['pre_own']))
    ref, bound = M.y_ref(d, f['act_own'])
    inside('y', f['y'], ref, bound, bound - A_BF * ref.abs())
    ref, bound, slack = M.dpre_ref(d)
    # (t is rounded to bf16 inside the chain: that rounding belongs to the rounding part, A_BF |ref| of the 2 A_BF |ref|)
    assert ratio((f['dpre'].double() - ref).abs(), 0.5 * slack + A_BF * ref.abs()) <= 1.0
    assert ratio((f['dpre_own'].double() - ref).abs(), bound) <= 1.0
    ref, bound, slack = M.dx_ref(d, f['dpre_own'], acc)
    inside('dx', f['dx'], ref, bound, slack)


@pytest.mark.parametrize('ws,heads', [(4, 3), (7, 8)])
def test_fp32_cpb_stays_inside_half_of_the_bounds(ws, heads):
    d = M.make_cpb(ws, heads, seed=ws + heads)
    ref, bound = M.cpb_fwd_ref(d['table'], d['index'])
    assert ratio((M.cpb_fwd_ref(d['table'], d['index'], torch.float32)[0].double() - ref).abs(), 0.5 * bound) <= 1.0
    for tr in (0, 1):
        ref, bound, slack = M.cpb_bwd_ref(d, tr)
        f32 = M.cpb_bwd_ref(d, tr, torch.float32)[0]
        # (fp32 rounds 1 - s absolutely, which the accumulation term does not model: mlp_rows_ref.cpb_cancel)
        assert ratio((f32.double() - ref).abs(), 0.5 * slack + M.cpb_cancel(d, tr)) <= 1.0
        assert ratio((f32.to(BF).double() - ref).abs(), bound) <= 1.0
    # a transposed index is rejected (the window index is not symmetric), by the forward and by the backward
    ref, bound = M.cpb_fwd_ref(d['table'], d['index'])
    assert ratio((M.cpb_fwd_ref(d['table'], d['index'].t().contiguous())[0] - ref).abs(), bound) > 1.0
    ref, bound, _ = M.cpb_bwd_ref(d, 0)
    assert ratio((M.cpb_bwd_ref(d, 1)[0] - ref).abs(), bound) > 1.0


@pytest.mark.parametrize('has_cls', [0, 1])
@pytest.mark.parametrize('nec', [0, 1])
def test_fp32_embed_stays_inside_half_of_the_bounds(has_cls, nec):
    e = M.make_embed(3, 5, 24, has_cls, seed=7)
    ref, slack = M.embed_fwd_ref(e, nec)
    f32 = M.embed_fwd_ref(e, nec, torch.float32)[0]
    # (the forward is ONE fp32 add: its slack is exactly that rounding and cannot be halved)
    assert ratio((f32.double() - ref).abs(), slack) <= 1.0
    assert ratio((f32.to(BF).double() - ref).abs(), A_BF * ref.abs() + slack) <= 1.0
    dpos, dcls, sp, sc = M.embed_bwd_ref(e, nec)
    dpos32, dcls32, _, _ = M.embed_bwd_ref(e, nec, torch.float32)
    assert ratio((dpos32.double() - dpos).abs(), 0.5 * sp) <= 1.0
    assert dpos.shape[0] == (e['p'] if nec else e['t'])
    if has_cls:
        assert ratio((dcls32.double() - dcls).abs(), 0.5 * sc) <= 1.0
        # accumulate treated as overwrite is rejected
        assert ratio((dcls - (dcls + e['dcls_prior'].double())).abs(), sc + U32 * e['dcls_prior'].double().abs()) > 1.0
    if nec and has_cls:
        # the position row off by one under no_embed_class is rejected
        wrong = M.embed_fwd_ref(e, nec, shift=1)[0]
        assert ratio((wrong - ref).abs(), A_BF * ref.abs() + slack) > 1.0


# ---- wrong variants do not pass -----------------------------------------------------------------------------------------------------
def test_tanh_gelu_is_rejected():
    x = finite_table(1e38)
    ref, bound = M.act_fwd_ref(1, x)
    err = (M.gelu_tanh(x).float().to(BF).double() - ref).abs()
    over = float((err > bound).double().mean())
    r = ratio(err, bound)
    assert r > 10 and over > 0.002, (r, over)                                                # measured: 31 x at x = -3.375, 0.25 %


@pytest.mark.parametrize('c', M.WIDTHS)
def test_wrong_mlp_variants_are_rejected(c):
    d = M.make_mlp(c, 77, seed=c + 2)
    f = M.mlp_fp32(d, 1)
    ref, bound = M.y_ref(d, f['act_own'])
    no_b2 = M.y_ref(d, f['act_own'], b2=False)[0].float().to(BF).double()
    assert ratio((no_b2 - ref).abs(), bound) > 1.0, 'a missing b2'
    ref, bound = M.act_ref(f['pre_own'])
    assert ratio((f['pre_own'].double() - ref).abs(), bound) > 1.0, 'act saved as pre'
    ref, bound, _ = M.dx_ref(d, f['dpre_own'], True)
    fresh = M.dx_ref(d, f['dpre_own'], False)[0].float().to(BF).double()
    assert ratio((fresh - ref).abs(), bound) > 1.0, 'accumulate treated as overwrite'
