"""Kernel contracts of the ReLU6 form of the mask-less activation path (csrc/bn.hip: tok_bn_relu6_fwd, tok_bn_relu6_bwd_reduce,
tok_bn_relu6_bwd_apply), element by element against fp64 torch on the same bf16 inputs.  Every operand sits between guard
regions (helpers.gin / gout): a read or write outside it fails the case.

z = y * scale + shift.  out = min(max(z, 0), 6);  dz = dout * [0 < z < 6], the interval open (aten::hardtanh_backward gives 0
at z == 0 and at z == 6);  dy = c1 * dz + c2 * y + c3."""
import pytest
import torch

from helpers import A_BF, BF, ERR_INVALID, F32, U32, assert_bounded, gin, gout, last_error, rel_err
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
GUARD = 4096
# |z - 0| or |z - 6| below this in fp64: fp32 may take the other branch of the derivative.  Ten times the largest fp32-vs-fp64
# difference of z on these inputs (9.5e-7: |y * scale| + |shift| <= 25, 2 ulp of it): no element outside the band changes branch
KINK_BAND = 1e-5
# (rows, channels): the smallest legal shape; rows no multiple of the rows per block; a small layer; the head of every
# EfficientNet-Lite; six times lite4's last width, more than 256 channel groups (the cg loop); 70 001 rows of 8 channels; and
# 1024 blocks x 256 rows + 257 rows of 8 channels, the size at which the 1024-block cap of both launch geometries is exceeded and
# the grid-stride loop runs a second trip
SHAPES = [(1, 8), (37, 16), (2 * 7 * 7, 72), (2 * 14 * 14, 1280), (300, 2688), (70001, 8), (1024 * 256 + 257, 8)]


def _inputs(m, c):
    g = torch.Generator().manual_seed(1000 * c + m % 997)
    y = torch.randn(m, c, generator=g).to(BF)
    dout = torch.randn(m, c, generator=g).to(BF)
    scale = 1.0 + 3.0 * torch.rand(c, generator=g)          # (random reals: no bf16 value of y lands on a kink exactly)
    shift = 4.0 * torch.rand(c, generator=g) - 1.0
    mean = y.float().mean(0) if m > 1 else torch.zeros(c)
    rstd = 1.0 / (y.float().var(0, unbiased=False) + 1e-5).sqrt() if m > 1 else torch.ones(c)
    gamma = (scale / rstd).contiguous()
    return y, dout, scale, shift, mean.contiguous(), rstd.contiguous(), gamma


def _relu6_d(z):
    return ((z > 0) & (z < 6)).to(z.dtype)


def _run(m, c, y, dout, scale, shift, mean, rstd, gamma, coef=None):
    """forward, reduce -> finalize, apply on the device; coef given: the apply alone on it (the eval form)"""
    lib, st = _C.lib(), stream_ptr()
    gy, gd = gin(y, GUARD), gin(dout, GUARD)
    vec = [gin(t, 64) for t in (scale, shift, mean, rstd)]
    out = gout(m * c, BF, GUARD)
    _C.check(lib.tok_bn_relu6_fwd(gy.ptr, vec[0].ptr, vec[1].ptr, out.ptr, m, c, st), 'fwd')
    rows = lib.tok_bn_bwd_rows(m, c)
    partial = gout(2 * rows * c, F32, GUARD)
    _C.check(lib.tok_bn_relu6_bwd_reduce(gd.ptr, gy.ptr, *(v.ptr for v in vec), m, c, partial.ptr, st), 'reduce')
    gam = gamma.cuda()
    if coef is None:
        co = gout(3 * c, F32, 64)
        _C.check(lib.tok_bn_bwd_finalize(partial.ptr, rows, m, c, c, gam.data_ptr(), vec[2].ptr, vec[3].ptr, None, None,
                                         co.ptr, 0, 0, st), 'finalize')
    else:
        co = gin(coef, 64)
    dy = gout(m * c, BF, GUARD)
    _C.check(lib.tok_bn_relu6_bwd_apply(gd.ptr, gy.ptr, vec[0].ptr, vec[1].ptr, co.ptr, dy.ptr, m, c, st), 'apply')
    torch.cuda.synchronize()
    for t, what in ((out, 'out'), (partial, 'partial'), (dy, 'dy'), (co, 'coef')):
        t.check(what)
    return (out.value().view(m, c), partial.value().view(2, rows, c), dy.value().view(m, c), co.value().view(3, c))


@pytest.mark.parametrize('m,c', SHAPES)
def test_relu6_forward_reduce_apply_vs_fp64(m, c):
    """out: |out - ref| <= 2^-8 |ref| + 4 u32 (|y scale| + |shift|), one bf16 rounding of the stored value plus the fp32 fma that
    forms z; exactly 0 where fp64 z <= -1e-5 and exactly 6.0 where z >= 6 + 1e-5.
    dy: |dy - ref| <= 2^-7 |ref| + 4 u32 (|c1 dz| + |c2 y| + |c3|): the bf16 store (one rounding is 2^-8) and the three fp32
    operations of c1*dz + c2*y + c3.  The hard-swish bound without its derivative-response term: this derivative is piecewise
    constant, so outside the kink band a z formed in fp32 gives the same dz.
    The folded reduce rows <= 1e-3 (relative L2).  Elements whose fp64 z lies within 1e-5 of a kink are left out of the dy
    check and enter the reduce reference with the branch of the fp32 z; their share is at most 0.1 %."""
    y, dout, scale, shift, mean, rstd, gamma = _inputs(m, c)
    out, partial, dy, coef = _run(m, c, y, dout, scale, shift, mean, rstd, gamma)
    yd, gd = y.double(), dout.double()
    z = yd * scale.double() + shift.double()
    shares = {'z <= 0': float((z <= 0).double().mean()), '0 < z < 6': float(((z > 0) & (z < 6)).double().mean()),
              'z >= 6': float((z >= 6).double().mean())}
    print(f'relu6 {m}x{c}: shares {shares}')
    if m * c >= 2 * 7 * 7 * 72:
        for what, share in shares.items():
            assert share >= 0.01, (what, share)
    ref_out = z.clamp(0, 6)
    mag_z = (yd * scale.double()).abs() + shift.double().abs()
    worst = assert_bounded(out, ref_out, mag_z, A_BF, 4 * U32, what=f'out {m}x{c}')
    assert bool((out[z <= -KINK_BAND] == 0).all()) and bool((out[z >= 6 + KINK_BAND] == 6.0).all())
    near = (z.abs() < KINK_BAND) | ((z - 6).abs() < KINK_BAND)
    share_near = float(near.double().mean())
    assert share_near <= 1e-3, share_near
    keep = ~near
    dz = gd * _relu6_d(z)
    xhat = (yd - mean.double()) * rstd.double()
    folded = partial.double().sum(1)
    # the sums cannot leave an element out: inside the band the reference takes the branch of z as the contract forms it, one
    # fp32 fma (y * scale is exact in fp64, so rounding the fp64 sum to fp32 is that fma), outside it the fp64 branch
    z_fma = z.float().double()
    dz_sum = torch.where(near, gd * _relu6_d(z_fma), dz)
    r0, r1 = rel_err(folded[0], dz_sum.sum(0)), rel_err(folded[1], (dz_sum * xhat).sum(0))
    print(f'relu6 {m}x{c}: out worst err/bound {worst:.3g}, kink share {share_near:.3g}, reduce rel err {r0:.3g} {r1:.3g}')
    assert r0 <= 1e-3 and r1 <= 1e-3, (r0, r1)
    c1, c2, c3 = coef.double()
    ref = c1 * dz + c2 * yd + c3
    mag = 4 * U32 * ((c1 * dz).abs() + (c2 * yd).abs() + c3.abs())
    worst = assert_bounded(dy[keep], ref[keep], mag[keep], 2 * A_BF, 1.0, what=f'dy {m}x{c}')
    print(f'relu6 {m}x{c}: dy worst err/bound {worst:.3g}')
    again = _run(m, c, y, dout, scale, shift, mean, rstd, gamma)
    for a, b in zip((out, partial, dy, coef), again):
        assert torch.equal(a, b)


def _exact_inputs(m, c):
    """scale from {0.5, 1, 2}, integer shift, small-integer y and dout: z = y * scale + shift is exact in fp32 and bf16, lies in
    [-9, 15] in steps of 0.5 and hits 0 and 6 exactly"""
    g = torch.Generator().manual_seed(3 * c + m)
    y = torch.randint(-4, 5, (m, c), generator=g).float().to(BF)
    dout = torch.randint(-8, 9, (m, c), generator=g).float().to(BF)
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c,), generator=g)].contiguous()
    shift = torch.randint(-1, 8, (c,), generator=g).float()
    return y, dout, scale, shift


@pytest.mark.parametrize('m,c', [(37, 16), (1031, 72)])
def test_relu6_exact_cases_bit_for_bit(m, c):
    """forward bit for bit; dz bit for bit with derivative 0 at both kinks: apply with coef = (1, 0, 0) returns dz itself, and the
    reduce rows fold to the integer sum of dz exactly"""
    y, dout, scale, shift = _exact_inputs(m, c)
    z = y.double() * scale.double() + shift.double()
    assert bool((z == 0).any()) and bool((z == 6).any()) and bool((z < 0).any()) and bool((z > 6).any())
    coef = torch.zeros(3, c)
    coef[0] = 1.0
    mean, rstd = torch.zeros(c), torch.ones(c)
    out, partial, dy, _ = _run(m, c, y, dout, scale, shift, mean, rstd, torch.ones(c), coef=coef)
    assert torch.equal(out, z.clamp(0, 6).to(BF))
    dz = dout.double() * _relu6_d(z)
    assert bool((dz[(z == 0) | (z == 6)] == 0).all())
    assert torch.equal(dy, dz.to(BF)) and torch.equal(dy.double(), dz)
    folded = partial.double().sum(1)                       # integers far below 2^24: every partial sum is exact
    assert torch.equal(folded[0], dz.sum(0)) and torch.equal(folded[1], (dz * y.double()).sum(0))


@pytest.mark.parametrize('m,c', [(37, 16), (2 * 14 * 14, 1280)])
def test_relu6_apply_eval_form(m, c):
    """coef = (scale, 0, 0): dy = scale * dz, the backward of a unit under eval-mode BatchNorm"""
    y, dout, scale, shift, mean, rstd, gamma = _inputs(m, c)
    coef = torch.zeros(3, c)
    coef[0] = scale
    _, _, dy, _ = _run(m, c, y, dout, scale, shift, mean, rstd, gamma, coef=coef)
    z = y.double() * scale.double() + shift.double()
    ref = scale.double() * dout.double() * _relu6_d(z)
    keep = ~((z.abs() < KINK_BAND) | ((z - 6).abs() < KINK_BAND))
    assert_bounded(dy[keep], ref[keep], (4 * U32 * ref.abs())[keep], 2 * A_BF, 1.0, what=f'eval dy {m}x{c}')


def test_relu6_refusals_launch_nothing():
    """c = 12, m = 0 and each null pointer of each entry point: TOK_ERR_INVALID, nothing written"""
    lib, st = _C.lib(), stream_ptr()
    out = gout(64, BF, 64)
    buf = torch.zeros(64, device='cuda')
    # (entry point, its pointer arguments: the inputs, then the output last)
    entries = [('tok_bn_relu6_fwd', 4), ('tok_bn_relu6_bwd_apply', 6), ('tok_bn_relu6_bwd_reduce', 7)]

    def call(name, n_ptr, m, c, null=None):
        a = [buf.data_ptr()] * (n_ptr - 1) + [out.ptr]
        if null is not None:
            a[null] = None
        if name == 'tok_bn_relu6_bwd_reduce':
            return lib.tok_bn_relu6_bwd_reduce(*a[:6], m, c, a[6], st)
        return getattr(lib, name)(*a, m, c, st)

    for name, n_ptr in entries:
        for m, c in ((4, 12), (0, 8), (4, 0)):
            assert call(name, n_ptr, m, c) == ERR_INVALID, (name, m, c)
            assert name in last_error()
        for null in range(n_ptr):
            assert call(name, n_ptr, 4, 8, null) == ERR_INVALID, (name, null)
            assert name in last_error()
    torch.cuda.synchronize()
    out.check('refusals')
    assert out.untouched()
