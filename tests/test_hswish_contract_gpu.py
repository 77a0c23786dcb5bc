"""Kernel contracts of the mask-less activation path (csrc/bn.hip: BatchNorm + hard-swish forward, backward reduce and
backward apply) and of the gated squeeze-excite entry points (csrc/se.hip), against fp64 torch on the same bf16 inputs.
Every operand sits between guard regions (helpers.gin / gout): a read or write outside it fails the case."""
import pytest
import torch
import torch.nn.functional as F

from helpers import A_BF, BF, ERR_INVALID, F32, U32, assert_bounded, gin, gout, last_error, rel_err
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
GUARD = 4096
KINK_BAND = 1e-3          # |z -+ 3| below this: fp32 and fp64 may take different branches of the derivative (a jump of 0.5)
# (rows, channels): the smallest legal shape; rows no multiple of the rows per block; a small and the widest MobileNetV3 layer;
# more than 256 channel groups (the cg loop); 70 001 rows of 8 channels; and 1024 blocks x 256 rows + 257 rows of 8 channels,
# the size at which the 1024-block cap of both launch geometries is exceeded and the grid-stride loop runs a second trip
SHAPES = [(1, 8), (37, 16), (2 * 7 * 7, 72), (2 * 14 * 14, 960), (300, 2176), (70001, 8), (1024 * 256 + 257, 8)]


def _inputs(m, c):
    g = torch.Generator().manual_seed(1000 * c + m % 997)
    y = torch.randn(m, c, generator=g).to(BF)
    dout = torch.randn(m, c, generator=g).to(BF)
    scale = 0.5 + 1.5 * torch.rand(c, generator=g)          # (random reals: no bf16 value of y lands on a kink exactly)
    shift = 2.0 * torch.rand(c, generator=g) - 1.0
    mean = y.float().mean(0) if m > 1 else torch.zeros(c)
    rstd = 1.0 / (y.float().var(0, unbiased=False) + 1e-5).sqrt() if m > 1 else torch.ones(c)
    gamma = (scale / rstd).contiguous()
    return y, dout, scale, shift, mean.contiguous(), rstd.contiguous(), gamma


def _hswish_d(z):
    return torch.where(z < -3, torch.zeros_like(z), torch.where(z <= 3, z / 3 + 0.5, torch.ones_like(z)))


def _run(m, c, y, dout, scale, shift, mean, rstd, gamma, coef=None):
    """forward, reduce -> finalize, apply on the device; coef given: the apply alone on it (the eval form)"""
    lib, st = _C.lib(), stream_ptr()
    gy, gd = gin(y, GUARD), gin(dout, GUARD)
    vec = [gin(t, 64) for t in (scale, shift, mean, rstd)]
    out = gout(m * c, BF, GUARD)
    _C.check(lib.tok_bn_hswish_fwd(gy.ptr, vec[0].ptr, vec[1].ptr, out.ptr, m, c, st), 'fwd')
    rows = lib.tok_bn_bwd_rows(m, c)
    partial = gout(2 * rows * c, F32, GUARD)
    _C.check(lib.tok_bn_hswish_bwd_reduce(gd.ptr, gy.ptr, *(v.ptr for v in vec), m, c, partial.ptr, st), 'reduce')
    gam = gamma.cuda()
    if coef is None:
        co = gout(3 * c, F32, 64)
        _C.check(lib.tok_bn_bwd_finalize(partial.ptr, rows, m, c, c, gam.data_ptr(), vec[2].ptr, vec[3].ptr, None, None,
                                         co.ptr, 0, 0, st), 'finalize')
    else:
        co = gin(coef, 64)
    dy = gout(m * c, BF, GUARD)
    _C.check(lib.tok_bn_hswish_bwd_apply(gd.ptr, gy.ptr, vec[0].ptr, vec[1].ptr, co.ptr, dy.ptr, m, c, st), 'apply')
    torch.cuda.synchronize()
    for t, what in ((out, 'out'), (partial, 'partial'), (dy, 'dy'), (co, 'coef')):
        t.check(what)
    return (out.value().view(m, c), partial.value().view(2, rows, c), dy.value().view(m, c), co.value().view(3, c))


@pytest.mark.parametrize('m,c', SHAPES)
def test_hswish_forward_reduce_apply_vs_fp64(m, c):
    """out <= 1e-2, the folded reduce rows <= 1e-3, dy <= 1e-2 (relative L2), then dy element by element:
    |dy - ref| <= 2^-7 |ref| + 4 u32 (|c1 dz| + |c2 y| + |c3|) + 1e-6 |c1 dout|.  The first term is the bf16 store (one rounding is
    2^-8), the second the three fp32 operations of c1*dz + c2*y + c3 and of dz, the third the derivative's response to
    z being formed in fp32 (2 ulp of |y*scale| + |shift| <= 9, a third of it in the middle branch).  Elements whose fp64 z lies
    within 1e-3 of a kink are left out of the element-wise check only; their share is at most 0.1 %."""
    y, dout, scale, shift, mean, rstd, gamma = _inputs(m, c)
    out, partial, dy, coef = _run(m, c, y, dout, scale, shift, mean, rstd, gamma)
    yd, gd = y.double(), dout.double()
    z = yd * scale.double() + shift.double()
    if m * c >= 2 * 7 * 7 * 72:
        for share, what in (((z < -3).double().mean(), 'z < -3'), ((z.abs() < 3).double().mean(), '|z| < 3'),
                            ((z > 3).double().mean(), 'z > 3')):
            assert float(share) >= 0.01, (what, float(share))
    assert rel_err(out, F.hardswish(z)) <= 1e-2
    dz = gd * _hswish_d(z)
    xhat = (yd - mean.double()) * rstd.double()
    folded = partial.double().sum(1)
    assert rel_err(folded[0], dz.sum(0)) <= 1e-3
    assert rel_err(folded[1], (dz * xhat).sum(0)) <= 1e-3
    c1, c2, c3 = coef.double()
    ref = c1 * dz + c2 * yd + c3
    assert rel_err(dy, ref) <= 1e-2
    near = ((z - 3).abs() < KINK_BAND) | ((z + 3).abs() < KINK_BAND)
    assert float(near.double().mean()) <= 1e-3
    keep = ~near
    mag = 4 * U32 * ((c1 * dz).abs() + (c2 * yd).abs() + c3.abs()) + 1e-6 * (c1 * gd).abs()
    assert_bounded(dy[keep], ref[keep], mag[keep], 2 * A_BF, 1.0, what=f'dy {m}x{c}')
    again = _run(m, c, y, dout, scale, shift, mean, rstd, gamma)
    for a, b in zip((out, partial, dy, coef), again):
        assert torch.equal(a, b)


@pytest.mark.parametrize('m,c', [(37, 16), (2 * 14 * 14, 960)])
def test_hswish_apply_eval_form(m, c):
    """coef = (scale, 0, 0): dy = scale * dz, the backward of a unit under eval-mode BatchNorm"""
    y, dout, scale, shift, mean, rstd, gamma = _inputs(m, c)
    coef = torch.zeros(3, c)
    coef[0] = scale
    _, _, dy, _ = _run(m, c, y, dout, scale, shift, mean, rstd, gamma, coef=coef)
    z = y.double() * scale.double() + shift.double()
    ref = scale.double() * dout.double() * _hswish_d(z)
    assert rel_err(dy, ref) <= 1e-2
    keep = ~(((z - 3).abs() < KINK_BAND) | ((z + 3).abs() < KINK_BAND))
    mag = 4 * U32 * ref.abs() + 1e-6 * (scale.double() * dout.double()).abs()
    assert_bounded(dy[keep], ref[keep], mag[keep], 2 * A_BF, 1.0, what=f'eval dy {m}x{c}')


def test_hswish_invalid_sizes_launch_nothing():
    lib, st = _C.lib(), stream_ptr()
    out = gout(64, BF, 64)
    buf = torch.zeros(64, device='cuda')
    for m, c in ((4, 12), (0, 8), (4, 0)):
        assert lib.tok_bn_hswish_fwd(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), out.ptr, m, c, st) == ERR_INVALID
        assert lib.tok_bn_hswish_bwd_apply(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), out.ptr,
                                           m, c, st) == ERR_INVALID
        assert lib.tok_bn_hswish_bwd_reduce(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(),
                                            buf.data_ptr(), m, c, out.ptr, st) == ERR_INVALID
        assert 'tok_bn_hswish' in last_error()
    torch.cuda.synchronize()
    assert out.untouched()


# ---- squeeze-excite with a gate argument ---------------------------------------------------------------------------------
SE_SHAPES = [(72, 6, 28), (120, 10, 15), (672, 28, 14), (960, 240, 7)]
SATURATION_STD = 1.82        # P(|N(0, 1.82^2)| > 3) = 0.1: about a tenth of the hard-sigmoid gates at 0 or 1


def _se_inputs(c, rd, hw, n=4):
    g = torch.Generator().manual_seed(c + rd)
    x = torch.randn(n, hw, hw, c, generator=g).abs().to(BF)
    w1, b1 = torch.randn(rd, c, generator=g) / c ** 0.5, torch.randn(rd, generator=g) * 0.1
    w2, b2 = torch.randn(c, rd, generator=g) / rd ** 0.5, torch.randn(c, generator=g) * 0.1
    a = F.relu(x.double().mean((1, 2)) @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double()
    k = SATURATION_STD / float(a.std())
    dout = torch.randn(n, hw, hw, c, generator=g).to(BF)
    return x, [w1.contiguous(), b1, (w2 * k).contiguous(), b2 * k], dout


def _se_ref(x, prm, dout, gate_fn):
    prm = [t.double().requires_grad_() for t in prm]
    xd = x.double().requires_grad_()
    hid = F.relu(xd.mean((1, 2)) @ prm[0].t() + prm[1])
    gate = gate_fn(hid @ prm[2].t() + prm[3])
    (xd * gate[:, None, None, :] * dout.double()).sum().backward()
    return gate.detach(), xd.grad, [p.grad for p in prm]


def _se_run(kind, x, prm, dout, acc_bits=0, dx_acc=0, prefill=None, entry='gate'):
    """kind: 0 sigmoid, 1 hard sigmoid; entry 'plain': tok_se_fwd / tok_se_bwd (sigmoid only).  prefill: (grads, dx) to start from."""
    lib, st = _C.lib(), stream_ptr()
    n, h, w, c = x.shape
    rd = prm[0].shape[0]
    xg, dg = gin(x, GUARD), gin(dout, GUARD)
    dev = [gin(t, 64) for t in prm]
    mean, hid, gate = gout(n * c, F32, 64), gout(n * rd, F32, 64), gout(n * c, F32, 64)
    ws = gout(lib.tok_se_ws_floats(n, h * w, c, rd), F32, GUARD)
    grads = [gout(t.numel(), F32, 64, init=None if prefill is None else prefill[0][i]) for i, t in enumerate(prm)]
    dx = gout(x.numel(), BF, GUARD, init=None if prefill is None else prefill[1])
    if entry == 'plain':
        _C.check(lib.tok_se_fwd(xg.ptr, n, h * w, c, c, rd, *(t.ptr for t in dev), mean.ptr, hid.ptr, gate.ptr, ws.ptr, st), 'fwd')
        _C.check(lib.tok_se_bwd(dg.ptr, xg.ptr, n, h * w, c, c, rd, dev[0].ptr, dev[2].ptr, mean.ptr, hid.ptr, gate.ptr,
                                *(t.ptr for t in grads), acc_bits, dx.ptr, dx_acc, ws.ptr, st), 'bwd')
    else:
        _C.check(lib.tok_se_gate_fwd(xg.ptr, n, h * w, c, c, rd, kind, *(t.ptr for t in dev), mean.ptr, hid.ptr, gate.ptr, ws.ptr,
                                     st), 'gate_fwd')
        _C.check(lib.tok_se_gate_bwd(dg.ptr, xg.ptr, n, h * w, c, c, rd, kind, dev[0].ptr, dev[2].ptr, mean.ptr, hid.ptr, gate.ptr,
                                     *(t.ptr for t in grads), acc_bits, dx.ptr, dx_acc, ws.ptr, st), 'gate_bwd')
    torch.cuda.synchronize()
    for t in [mean, hid, gate, ws, dx] + grads:
        t.check('se')
    return [gate.value().view(n, c), dx.value().view(x.shape)] + [t.value().view(p.shape) for t, p in zip(grads, prm)]


@pytest.mark.parametrize('c,rd,hw', SE_SHAPES)
def test_se_hard_sigmoid_gate_vs_fp64(c, rd, hw):
    x, prm, dout = _se_inputs(c, rd, hw)
    gate_ref, dx_ref, grad_ref = _se_ref(x, prm, dout, F.hardsigmoid)
    saturated = float(((gate_ref == 0) | (gate_ref == 1)).double().mean())
    assert 0.02 <= saturated <= 0.5, saturated
    mine = _se_run(1, x, prm, dout)
    assert rel_err(mine[0], gate_ref) <= 1e-3
    assert rel_err(mine[1], dx_ref) <= 1e-2
    for got, ref in zip(mine[2:], grad_ref):
        assert rel_err(got, ref) <= 1e-3
    for a, b in zip(mine, _se_run(1, x, prm, dout)):
        assert torch.equal(a, b)
    # each accumulate bit adds onto its pre-filled target and leaves the others to be overwritten
    g = torch.Generator().manual_seed(7)
    fill = [torch.randn(t.shape, generator=g) for t in prm]
    fill_dx = torch.randn(x.shape, generator=g).to(BF)
    for bit in range(4):
        got = _se_run(1, x, prm, dout, acc_bits=1 << bit, prefill=(fill, fill_dx))
        for i in range(4):
            want = grad_ref[i] + fill[i].double() if i == bit else grad_ref[i]
            assert rel_err(got[2 + i], want) <= 1e-3, (bit, i)
        assert torch.equal(got[1], mine[1])
    got = _se_run(1, x, prm, dout, dx_acc=1, prefill=(fill, fill_dx))
    assert rel_err(got[1], dx_ref + fill_dx.double()) <= 1e-2
    assert all(torch.equal(a, b) for a, b in zip(got[2:], mine[2:]))


@pytest.mark.parametrize('c,rd,hw', SE_SHAPES)
def test_se_sigmoid_entries_are_unchanged(c, rd, hw):
    """tok_se_fwd / tok_se_bwd on the same inputs still give what the fp64 sigmoid reference says, and gate 0 of the new entry
    points is those kernels: the same bits."""
    x, prm, dout = _se_inputs(c, rd, hw)
    gate_ref, dx_ref, grad_ref = _se_ref(x, prm, dout, torch.sigmoid)
    plain = _se_run(0, x, prm, dout, entry='plain')
    assert rel_err(plain[0], gate_ref) <= 1e-3
    assert rel_err(plain[1], dx_ref) <= 1e-2
    for got, ref in zip(plain[2:], grad_ref):
        assert rel_err(got, ref) <= 1e-3
    for a, b in zip(plain, _se_run(0, x, prm, dout)):
        assert torch.equal(a, b)


@pytest.mark.parametrize('c', [12, 2056])
def test_se_invalid_sizes_launch_nothing(c):
    lib, st = _C.lib(), stream_ptr()
    n, hw, rd = 2, 4, 8
    buf = torch.zeros(n * hw * 2064, device='cuda')
    outs = [gout(n * 2064, F32, 64) for _ in range(3)]
    p = buf.data_ptr()
    assert lib.tok_se_gate_fwd(p, n, hw, c, c, rd, 1, p, p, p, p, *(o.ptr for o in outs), p, st) == ERR_INVALID
    assert 'tok_se_gate_fwd' in last_error()
    assert lib.tok_se_gate_bwd(p, p, n, hw, c, c, rd, 1, p, p, p, p, p, *(o.ptr for o in outs), None, 0, None, 0, p, st) == ERR_INVALID
    assert 'tok_se_gate_bwd' in last_error()
    assert lib.tok_se_gate_fwd(p, n, hw, 16, 16, rd, 2, p, p, p, p, *(o.ptr for o in outs), p, st) == ERR_INVALID   # unknown gate
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)
