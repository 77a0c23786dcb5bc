"""tests/pool_ref.py against ATen on the CPU, on every shape list and input family of tests/test_pool_contract_gpu.py: the
references the device is held to are torch's operations, not this project's reading of them."""
import pytest
import torch
import torch.nn.functional as F

import pool_ref as R

F64 = torch.float64


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# the shapes past the grid cap run the tie family only, here and on the device
@pytest.mark.parametrize('shape,family', [(s, f) for s in R.MAXPOOL_SHAPES for f in R.FAMILIES] +
                         [(R.MAXPOOL_FWD_BIG, 'ties'), (R.MAXPOOL_BWD_BIG, 'ties')], ids=str)
def test_maxpool_is_aten(shape, family):
    n, h, w, c = shape
    x = R.maxpool_input(shape, family)
    best, tap = R.maxpool_fwd(x)
    xa = _nchw(x.double()).requires_grad_(True)
    ya, ia = F.max_pool2d(xa, 3, 2, 1, return_indices=True)
    assert torch.equal(tap, R.tap_from_flat(ia, h, w))
    assert 0 <= int(tap.min()) and int(tap.max()) <= 8
    assert torch.equal(best.isnan(), _nhwc(ya).isnan())
    assert torch.equal(best.nan_to_num(nan=7.0), _nhwc(ya.detach()).nan_to_num(nan=7.0))
    if family == 'ties':
        assert bool(((best[..., None] == x.double().new_tensor([-1.5, -0.5, 0.5, 1.5])).any(-1)).all())
    if family == 'neginf':
        assert bool((best[0, 0, 0] == float('-inf')).all())          # a window that sees -inf alone
    dy = torch.randint(-4, 5, best.shape, generator=torch.Generator().manual_seed(1)).double()
    ya.backward(_nchw(dy))
    assert torch.equal(R.maxpool_bwd(dy, tap, h, w), _nhwc(xa.grad))


@pytest.mark.parametrize('shape', R.AVGPOOL_SHAPES, ids=str)
def test_avgpool_is_aten(shape):
    n, h, w, c = shape
    for x in (torch.randn(shape, generator=torch.Generator().manual_seed(h * 9 + w)).to(R.BF), R.avg_exact_input(shape)):
        xa = _nchw(x.double()).requires_grad_(True)
        ya = F.avg_pool2d(xa, 2, 2, ceil_mode=True, count_include_pad=False)
        ref = R.avgpool_fwd(x)
        assert torch.allclose(ref, _nhwc(ya.detach()), rtol=1e-14, atol=0)
        dy = torch.randn(ref.shape, generator=torch.Generator().manual_seed(2), dtype=F64)
        ya.backward(_nchw(dy))
        assert torch.allclose(R.avgpool_bwd(dy, h, w), _nhwc(xa.grad), rtol=1e-14, atol=0)
    # the exact family: every window sum and every quotient survives a trip through bf16
    xe = R.avg_exact_input(shape).double()
    P, Q = R.pooled(h), R.pooled(w)
    xp = torch.zeros(n, 2 * P, 2 * Q, c, dtype=F64)
    xp[:, :h, :w] = xe
    sums = xp.view(n, P, 2, Q, 2, c).sum((2, 4))
    for t in (sums, R.avgpool_fwd(xe)):
        assert torch.equal(t.to(R.BF).double(), t)
    ge = R.avgpool_bwd(xe[:, ::2, ::2], h, w)                       # a gradient of the same family: quotients by 1, 2, 4
    assert torch.equal(ge.to(R.BF).double(), ge)


def _pix(x):                       # [n][hw][c] -> NCHW [n][c][hw][1]
    return x.permute(0, 2, 1).unsqueeze(-1).contiguous()


@pytest.mark.parametrize('shape', R.GAP_SHAPES + [R.GAP_BWD_BIG], ids=str)
def test_gap_is_aten(shape):
    n, hw, c = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(hw + c)).to(R.BF)
    xa = _pix(x.double()).requires_grad_(True)
    ya = F.adaptive_avg_pool2d(xa, 1)
    assert torch.allclose(R.gap_fwd(x), ya.detach().view(n, c), rtol=1e-13, atol=0)
    dy = torch.randn(n, c, generator=torch.Generator().manual_seed(3), dtype=F64)
    ya.backward(dy.view(n, c, 1, 1))
    assert torch.allclose(R.gap_bwd(dy, hw), xa.grad.squeeze(-1).permute(0, 2, 1), rtol=1e-14, atol=0)


@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('shape', R.GAP_SHAPES, ids=str)
def test_global_pool_is_aten(shape, family):
    n, hw, c = shape
    x = R.global_input(n, hw, c, family)
    mx, am = R.global_max(x)
    xa = _pix(x.double()).requires_grad_(True)
    ym, im = F.adaptive_max_pool2d(xa, 1, return_indices=True)
    assert torch.equal(am, im.view(n, c))
    assert torch.equal(mx.nan_to_num(nan=7.0), ym.detach().view(n, c).nan_to_num(nan=7.0))
    if family == 'neginf':
        assert float(mx[0, 0]) == float('-inf') and int(am[0, 0]) == 0
    if family == 'nan':
        return                     # the gradients below are compared on finite inputs
    ya = F.adaptive_avg_pool2d(xa, 1)
    g = torch.Generator().manual_seed(4)
    dy = torch.randn(n, 2 * c, generator=g, dtype=F64)
    outs = {1: (ym.view(n, c), dy[:, :c]), 2: (0.5 * (ya + ym).view(n, c), dy[:, :c]),
            3: (torch.cat([ya.view(n, c), ym.view(n, c)], 1), dy)}
    for mode, (y, gy) in outs.items():
        xa.grad = None
        y.backward(gy, retain_graph=True)
        dx, mag = R.global_pool_bwd(dy, am, hw, mode)
        assert torch.allclose(dx, xa.grad.squeeze(-1).permute(0, 2, 1), rtol=1e-13, atol=1e-300), mode
        assert bool((mag >= dx.abs() * (1 - 1e-14)).all())
    if family == 'ties':
        assert torch.allclose(R.avgmax_ref(x), outs[2][0].detach(), rtol=1e-13, atol=1e-300)


@pytest.mark.parametrize('shape', R.GAP_SHAPES, ids=str)
def test_avgmax_exact_family_is_representable(shape):
    n, hw, c = shape
    x = R.avgmax_exact_input(n, hw, c)
    avg, (mx, _) = R.gap_fwd(x), R.global_max(x)
    assert torch.equal(x.double().sum(1), avg * hw) and torch.equal(avg, avg.round())
    for t in (avg, mx, avg + mx, 0.5 * (avg + mx)):
        assert torch.equal(t.to(R.BF).double(), t)
    a, rest = R.avgmax_bound(x)
    assert a > 0 and bool((rest >= 0).all())


def test_colsum_partial_reference_and_launch_arithmetic():
    for m in R.PARTIAL_M + [R.PARTIAL_TALL[0]]:
        g, chunk = R.partial_rows(m)
        assert g == min(1024, -(-m // 256)) and g * chunk >= m
        assert (g - 1) * chunk < m or m == R.PARTIAL_TALL[0]            # every block owns a row, except at the tall shape
        x = torch.randint(-4, 5, (m, 8)).to(R.BF)
        rows, mag = R.colsum_partial(x, g, chunk)
        assert torch.equal(rows.sum(0), x.double().sum(0)) and torch.equal(mag.sum(0), x.double().abs().sum(0))
    g, chunk = R.partial_rows(R.PARTIAL_TALL[0])
    assert (g, chunk) == (1024, 257) and (g - 3) * chunk >= R.PARTIAL_TALL[0]          # three blocks own no row
    assert R.partial_launch(8)[2] == 256
    assert R.partial_launch(288) == (36, 36, 7, 4, 7 * 288 * 4)
    assert R.partial_launch(2048)[1:3] == (256, 1)
    assert R.partial_launch(3072)[0] > 256
    assert R.partial_launch(16384)[4] == 64 * 1024 and R.partial_launch(16392)[4] > 64 * 1024
