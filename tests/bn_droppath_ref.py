"""fp64 reference of the stochastic-depth BatchNorm trio of csrc/bn_droppath.hip (include/tok.h: tok_bn_droppath_fwd / _bwd_reduce /
_bwd_apply) on the same bf16 inputs and fp32 parameters, and the bounds of the contract, derived the way tests/bn_ref.py derives
those of tok_bn_act_fwd / tok_bn_bwd_reduce / tok_bn_bwd_apply with ONE MORE fp32 rounding for the product with s.
u32 = 2^-24, one bf16 rounding = 2^-8; an fp32 count is the number of roundings of the unfused formula and a bound takes twice
that count (bn_ref.py), so that any association, fused or not, sits inside half of it.

  out   = relu(s (y scale + shift) + shortcut)
          |err| <= 2^-8 |ref| + 8 u32 (|s| (|y scale| + |shift|) + |shortcut|)            (mul, add, mul, add: 4; one bf16 store)
          ReLU is a contraction: no element is left out.  mask = (stored out > 0), exactly.
  dt    = dout where the GIVEN mask bit is set: the mask is an input, nothing is left out.      dshortcut = dt exact;
          += : 2^-8 |ref| + 2 u32 (|dt| + |old|)
  dz    = s dt                                                                                 (1 rounding)
  sums  |err| <= (T + rpb + 4) u32 sum|term|    T trips of the row loop, rpb rows of a block, 4 = forming one term (the
          product with s, then sub, mul, mul); partial rows folded in fp64 by the test (bn_ref.n_sum + 1)
  dy    = c1 dz + c2 y + c3     |err| <= 2^-8 |ref| + 10 u32 (|c1 dz| + |c2 y| + |c3|)     (mul, mul, mul, add, add: 5)
          a dropped sample (s = 0): dz = 0 and dy = c2 y + c3, which the bound above holds to 10 u32 (|c2 y| + |c3|) + 2^-8 |ref|

INTEGER run: the operands of bn_ref.stream_inputs(integer=True) and s in {0, 1, 1.25, 2, 4}: every fp32 product, fma and partial
sum is exact (assert_exact: a partial row stays below 2^24 units of 1/32, the last place of a term), so each result is the fp64
one rounded ONCE to its storage format: out and dy carry up to 10 significant bits, more than bf16's 8, and the single bf16
rounding of the exact value is what the kernel must produce, bit for bit.

The chain fwd -> reduce -> tok_bn_bwd_finalize -> apply on the device's own intermediates: ChainRef below, bn_ref.ChainRef's
propagation with the factor s in z and dz."""
import torch

import bn_ref as B
from helpers import A_BF, BF, U32, assert_bounded, cdiv, pack_bits

F64 = torch.float64
B_OUT, B_DY, B_DS = 8 * U32, 10 * U32, 2 * U32
S_INT = [0.0, 1.0, 1.25, 2.0, 4.0]
S_REAL = [0.0, 1 / 0.9, 1 / 0.5]

# (n, rows_per_sample, c): see tests/test_bn_droppath_contract_gpu.py
SHAPES = [(1, 1, 8), (3, 5, 16), (4, 49, 24), (7, 1, 2048), (3, 100, 2176), (5, 257, 8), (2, 1024 * 128 + 3, 8)]


def n_sum(m, c):
    return B.n_sum(m, c) + 1


def draw_scale(n, integer, seed=0, mode='mixed'):
    """the per-sample factors as the fp32 values the kernel is handed.  mixed: every value of the set appears where n allows,
    sample 0 kept; 'ones': s == 1; 'zeros': every sample dropped; 'one_dropped': sample n // 2 dropped, the others 1 / keep"""
    vals = S_INT if integer else S_REAL
    g = torch.Generator().manual_seed(977 * seed + n)
    if mode == 'ones':
        return torch.ones(n)
    if mode == 'zeros':
        return torch.zeros(n)
    if mode == 'one_dropped':
        s = torch.full((n,), vals[-1], dtype=torch.float32)
        s[n // 2] = 0.0
        return s
    s = torch.tensor(vals, dtype=torch.float32)[torch.randint(0, len(vals), (n,), generator=g)]
    s[:min(n, len(vals))] = torch.tensor(vals[::-1], dtype=torch.float32)[:min(n, len(vals))]       # 1 / keep first, then down to 0
    return s.contiguous()


def inputs(n, rps, c, integer, seed=0, mode='mixed'):
    d = B.stream_inputs(n * rps, c, integer, seed)
    d['s'] = draw_scale(n, integer, seed, mode)
    d['dims'] = (n, rps, c)
    return d


class DropRef:
    def __init__(self, d):
        n, rps, c = d['dims']
        self.d = d
        y, sc, sh, s0 = d['y'].double(), d['scale'].double(), d['shift'].double(), d['shortcut'].double()
        self.s = d['s'].double().repeat_interleave(rps).view(n * rps, 1)
        self.z = y * sc + sh
        t = self.s * self.z + s0
        self.out = t.clamp_min(0)
        self.m_out = self.s.abs() * ((y * sc).abs() + sh.abs()) + s0.abs()
        self.pattern = t > 0
        self.mask_bytes = pack_bits(self.pattern)

    def bwd(self, pattern, acc):
        """with the mask the backward calls are handed (a bool [m][c])"""
        d = self.d
        y, g = d['y'].double(), d['dout'].double()
        dt = g * pattern
        dz = self.s * dt
        xh = (y - d['mean'].double()) * d['rstd'].double()
        c1, c2, c3 = d['coef'].double()
        r = dict(dt=dt, dz=dz, sums=torch.stack([dz.sum(0), (dz * xh).sum(0)]),
                 m_sums=torch.stack([dz.abs().sum(0), (dz * xh).abs().sum(0)]), terms=torch.stack([dz, dz * xh]),
                 dy=c1 * dz + c2 * y + c3, m_dy=(c1 * dz).abs() + (c2 * y).abs() + c3.abs(),
                 dy_dropped=c2 * y + c3, m_dy_dropped=(c2 * y).abs() + c3.abs())
        r['ds'] = dt + d['ds0'].double() if acc else dt
        r['m_ds'] = dt.abs() + d['ds0'].double().abs() if acc else torch.zeros_like(dt)
        return r


def assert_exact(d, b):
    """the integer run: every term is a multiple of 1/32 and a partial row (trips x rpb terms) stays below 2^24 of them"""
    n, rps, c = d['dims']
    m = n * rps
    per = cdiv(m, B.part_rows(m, c) * B.geo(c)[2]) * B.geo(c)[2]
    t = b['terms']
    assert bool((t * 32 == (t * 32).round()).all())
    assert per * float(t.abs().max()) * 32 < 2 ** 24


def bf_round(t):
    """one bf16 rounding of an fp64 value that fp32 holds exactly (the integer run)"""
    assert bool((t.float().double() == t).all())
    return t.float().to(BF).double()


def check_out(tag, ref, out, integer, frac=1.0):
    if integer:
        return B._eq(out, bf_round(ref.out), 'out')
    assert_bounded(out, ref.out, ref.m_out, A_BF if frac == 1.0 else 0.0, frac * B_OUT, 'out', tag if frac == 1.0 else None)


def check_mask(out, mask_bits):
    assert torch.equal(mask_bits, out.float() > 0), 'mask bits differ from (stored out > 0)'


def check_sums(tag, mine, b, m, c, integer, frac=1.0):
    """mine: the partial rows folded in fp64, [2][c]"""
    if integer:
        return B._eq(mine, b['sums'], 'bwd_reduce')
    for i, name in enumerate(('s1', 's2')):
        assert_bounded(mine[i], b['sums'][i], frac * n_sum(m, c) * U32 * b['m_sums'][i], 0.0, 1.0, f'bwd_reduce_{name}',
                       tag if frac == 1.0 else None)


def check_apply(tag, b, dy, ds, acc, integer, frac=1.0):
    rec = tag if frac == 1.0 else None
    a = A_BF if frac == 1.0 else 0.0
    if integer:
        B._eq(dy, bf_round(b['dy']), 'dy')
        if ds is not None:
            B._eq(ds, bf_round(b['ds']), 'dshortcut')
        return
    assert_bounded(dy, b['dy'], b['m_dy'], a, frac * B_DY, 'dy', rec)
    if ds is not None and acc:
        assert_bounded(ds, b['ds'], b['m_ds'], a, frac * B_DS, 'dshortcut', rec)
    elif ds is not None:
        B._eq(ds, b['ds'], 'dshortcut (a masked copy: exact)')


def fp32_run(d, pattern, acc):
    """the kernels' formulas in plain fp32 torch, unfused, before the bf16 stores; sums in the kernel's partition"""
    n, rps, c = d['dims']
    m = n * rps
    y = d['y'].float()
    s = d['s'].repeat_interleave(rps).view(m, 1)
    out = (s * (y * d['scale'] + d['shift']) + d['shortcut'].float()).clamp_min(0)
    dt = d['dout'].float() * pattern
    dz = s * dt
    xh = (y - d['mean']) * d['rstd']
    c1, c2, c3 = d['coef']
    return dict(out=out, sums=torch.stack([B.fp32_sum(dz, m, c), B.fp32_sum(dz * xh, m, c)]), dy=c1 * dz + c2 * y + c3,
                ds=dt + d['ds0'].float() if acc else dt)


def autograd_fp64(d, gamma, beta):
    """plain torch autograd in fp64 of out = relu(s * batch_norm(y) + shortcut) (training statistics) against upstream dout:
    out, mean, rstd, scale, shift and the gradients of y, shortcut, gamma and beta"""
    n, rps, c = d['dims']
    y = d['y'].double().requires_grad_(True)
    s0 = d['shortcut'].double().requires_grad_(True)
    ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = torch.nn.functional.batch_norm(y, None, None, ga, be, True, 0.0, B.EPS)
    out = torch.relu(d['s'].double().repeat_interleave(rps).view(-1, 1) * z + s0)
    dy, ds, dg, db = torch.autograd.grad(out, (y, s0, ga, be), d['dout'].double())
    mu = y.detach().mean(0)
    rstd = (y.detach().var(0, unbiased=False) + B.EPS) ** -0.5
    return dict(out=out.detach(), dy=dy, ds=ds, dgamma=dg, dbeta=db, mean=mu, rstd=rstd, scale=gamma.double() * rstd,
                shift=beta.double() - mu * gamma.double() * rstd)


class ChainRef:
    """fwd -> bwd_reduce -> tok_bn_bwd_finalize -> bwd_apply on the device's own intermediates (statistics by tok_bn_stats ->
    tok_bn_finalize) against fp64 training BatchNorm with the per-sample factor and its gradient.  bn_ref.ChainRef's error
    propagation with |s| in front of z and dz: the statistics are those of the un-dropped y and carry the same errors."""

    def __init__(self, d, gamma, beta):
        n, rps, c = d['dims']
        m = n * rps
        N = n_sum(m, c) * U32
        yd, g, b = d['y'].double(), gamma.double(), beta.double()
        s0, dout = d['shortcut'].double(), d['dout'].double()
        s = d['s'].double().repeat_interleave(rps).view(m, 1)
        mu = yd.mean(0)
        var = ((yd - mu) ** 2).mean(0)
        rstd = (var + B.EPS) ** -0.5
        scale, shift = g * rstd, b - mu * g * rstd
        e_mu = N * yd.abs().mean(0) + 2 * U32 * mu.abs()
        e_var = N * (yd * yd).mean(0) + 2 * mu.abs() * e_mu
        b_rstd = rstd * (8 * U32 + 0.5 * e_var / (var + B.EPS))
        b_scale = g.abs() * b_rstd + 2 * U32 * scale.abs()
        b_shift = mu.abs() * b_scale + scale.abs() * e_mu + 4 * U32 * ((mu * scale).abs() + b.abs())
        t = s * (yd * scale + shift) + s0
        self.out = t.clamp_min(0)
        self.m_out = s.abs() * ((yd * scale).abs() + shift.abs()) + s0.abs()
        self.e_out = s.abs() * (yd.abs() * b_scale + b_shift)
        self.near = t.abs() <= 2 * U32 * self.m_out + self.e_out          # the device's own pattern may differ here
        dz = s * dout * (t > 0)
        xh = (yd - mu) * rstd
        e_xh = rstd * e_mu + (yd - mu).abs() * b_rstd
        loose = s.abs() * dout.abs() * self.near
        s1, s2 = dz.sum(0), (dz * xh).sum(0)
        e_s1 = N * dz.abs().sum(0) + loose.sum(0)
        e_s2 = N * (dz * xh).abs().sum(0) + (dz.abs() * e_xh).sum(0) + (loose * (xh.abs() + e_xh)).sum(0)
        c1 = g * rstd
        c2 = -c1 * rstd * s2 / m
        c3 = -c1 * s1 / m - c2 * mu
        b_c1 = g.abs() * b_rstd + 2 * U32 * c1.abs()
        b_c2 = 8 * U32 * c2.abs() + (c1 * rstd).abs() * e_s2 / m + (s2 / m).abs() * (b_c1 * rstd + c1.abs() * b_rstd)
        b_c3 = mu.abs() * b_c2 + c2.abs() * e_mu + c1.abs() * e_s1 / m + (s1 / m).abs() * b_c1 + 8 * U32 * ((c2 * mu).abs() + (c1 * s1 / m).abs())
        self.dy = c1 * dz + c2 * yd + c3
        self.m_dy = (c1 * dz).abs() + (c2 * yd).abs() + c3.abs()
        self.e_dy = dz.abs() * b_c1 + yd.abs() * b_c2 + b_c3
        self.ds = dout * (t > 0)

    def check(self, tag, out, dy, ds):
        B._near_ok(self.near, 'chain')
        k = ~self.near
        assert_bounded(out, self.out, B_OUT * self.m_out + (1 + A_BF) * self.e_out, A_BF, 1.0, 'out', tag)      # ReLU contracts: all
        assert_bounded(dy[k], self.dy[k], (B_DY * self.m_dy + (1 + A_BF) * self.e_dy)[k], A_BF, 1.0, 'dy', tag)
        B._eq(ds[k], self.ds[k], 'dshortcut')
