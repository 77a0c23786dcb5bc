"""fp64 references of the training BatchNorm chain and the fused stem of csrc/bn.hip (include/tok.h) on the same bf16 inputs
and fp32 parameters, the bounds of the contract, and a plain fp32 run of the same formulas (tests/test_bn_ref.py: it stays
inside half of every bound).  u32 = 2^-24 (fp32 unit roundoff), one bf16 rounding = 2^-8.

Every kernel is run twice.  INTEGER run: y / shortcut / dout / dpool are integers in [-4, 4], scale in {1/2, 1, 2, 4}, shift a
half-integer (an odd quarter where scale = 1/2: z is never 0), mean a small integer, rstd in {1/2, 1, 2}, the apply coefficients dyadic: every fp32 product, fma and partial sum
is exact in any order (sums stay below 2^24 units of their last place: assert_exact_sums), so the result is the fp64 one bit
for bit.  REAL run: the bounds below.  An fp32 count is the number of roundings of the UNFUSED fp32 formula (a * b + c is two),
and a bound takes TWICE that count, so that an fp32 evaluation in any association, fused or not, sits inside half of it.

  out      |err| <= 2^-8 |ref| + 6 u32 (|y scale| + |shift| + |shortcut|)              (mul, add, add: 3; one bf16 store)
  sums     |err| <= (T + rpb + 3) u32 sum|term|   T = trips of the row loop, rpb = rows of a block (the shared-memory fold),
           3 = forming one term (sub, mul, mul);  the partial rows are folded in fp64 by the test.  Sequential fp32 sums: this
           is the worst case itself, not twice it; an fp32 run in this order stays inside half because roundings do not all
           push one way (checked on the CPU at every shape)
  colsum   the same on the kernel's OWN stored bf16 values (T + rpb roundings)
  dy       |err| <= 2^-8 |ref| + 8 u32 (|c1 dz| + |c2 y| + |c3|)                          (mul, mul, add, add: 4)
  dshortcut = dz: exact.  += : 2^-8 |ref| + 2 u32 (|dz| + |old|)                         (add: 1)
  ReLU pattern recomputed from y (mask == NULL) or taken from z in the reference: elements with |z| <= 2 u32 (|y scale| +
           |shift| + |shortcut|) (twice the rounding of z) may fall on either side.  They are left out element-wise, their
           terms are added to the bound of a sum, and their share stays under 0.1 % (asserted).  A mask that is GIVEN is an
           input: nothing is left out.
  finalize (fp64 fold of fp32 rows on both sides; e_var = (rows + 4) 2^-52 (S2 / n + mu^2): the fp64 cancellation)
    mean   2 u32 |mu|                                                                      (one cast)
    rstd   rstd (8 u32 + e_var / (2 (var + eps)))                                     (cast, add, sqrt, divide: 4)
    scale  |gamma| b_rstd + 2 u32 |scale|;   shift  |mu| b_scale + |scale| b_mean + 4 u32 (|mu scale| + |beta|)
    running_mean  momentum b_mean + 8 u32 (|momentum mu| + |(1 - momentum) rm|)            (1 - m, mul, mul, add: 4)
    running_var   momentum unbias e_var + 8 u32 (momentum unbias var + |(1 - momentum) rv|)
    dbeta  2 u32 |S1|;   dgamma  2 u32 |s2| + e_s2  (+ 2 u32 (|old| + |new|) under accumulate);  e_s2 = 0 in the xhat form,
           (rows + 4) 2^-52 rstd (sum|dz y| + |mu| sum|dz|) in the dz y form
    c1     2 u32 |c1|;   c2  8 u32 |c2| + |c1 rstd| e_s2 / m      (c1, mean cast, mul, mul: 4)
    c3     |mu| b_c2 + 8 u32 (|c2 mu| + |c1 S1 / m|)
  stem     pooled: 2^-8 |ref| + 6 u32 mag (ref = the fp64 value of the tap the kernel names, and the fp64 max);  ypool exact;
           d(z) of a position that two or more windows name is their fp32 sum (3 adds) rounded to bf16, as
           tok_maxpool3x3s2_bwd stores it:  e_g = 2^-8 |g| + 6 u32 sum|terms| there, 0 elsewhere;  sums += sum e_g (|xhat|),
           dy += |c1| e_g

No correct output uses more than half of the fp32 part of a bound; a bf16 output uses up to all of its 2^-8 |ref| term
whenever the exact value falls half way between two bf16 numbers."""
import torch

from helpers import A_BF, BF, U32, assert_bounded, cdiv, pack_bits

EPS, MOMENTUM = 1e-5, 0.1
CAP = 1024
NEAR_SHARE = 1e-3
B_OUT, B_DY, B_DS = 6 * U32, 8 * U32, 2 * U32
F64 = torch.float64

# (m, c) of the streaming kernels: see tests/test_bn_contract_gpu.py
STREAM_SHAPES = [(1, 8), (37, 16), (171, 24), (98, 72), (777, 48), (300, 2040), (300, 2048), (300, 2176), (1027, 2048),
                 (70001, 8), (1024 * 256 + 257, 8)]
STEM_SHAPES = [(1, 1, 1, 8), (1, 2, 3, 8), (2, 7, 9, 16), (3, 8, 8, 64), (1, 15, 17, 8), (3, 57, 61, 256)]
FINALIZE_ROWS = {c: (1, 3, 63, 64, 65, 256, 257, 512, 513, 1024) for c in (8, 48, 264)}
FINALIZE_ROWS.update({c: (1, 15, 16, 17, 64, 65, 128, 129, 1024) for c in (512, 520, 2048)})


def geo(c):
    cg = c // 8
    cge = min(cg, 256)
    return cg, cge, 256 // cge


def part_rows(m, c):
    return min(cdiv(m, geo(c)[2]), CAP)


def n_sum(m, c):
    rpb = geo(c)[2]
    return cdiv(m, part_rows(m, c) * rpb) + rpb + 3


def bf(t):
    return t.float().to(BF)


# ---- streaming kernels ---------------------------------------------------------------------------------------------------
def stream_inputs(m, c, integer, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + 31 * c + m % 9973 + (1 if integer else 0))
    r = lambda *s: torch.randn(*s, generator=g)                   # noqa: E731
    pick = lambda vals, n: torch.tensor(vals)[torch.randint(0, len(vals), (n,), generator=g)]       # noqa: E731
    if integer:
        ints = lambda: torch.randint(-4, 5, (m, c), generator=g).to(BF)       # noqa: E731
        d = dict(y=ints(), shortcut=ints(), dout=ints(), ds0=ints(),
                 scale=pick([0.5, 1.0, 2.0, 4.0], c), shift=torch.randint(-4, 4, (c,), generator=g).float() + 0.5,
                 mean=torch.randint(-2, 3, (c,), generator=g).float(), rstd=pick([0.5, 1.0, 2.0], c),
                 coef=torch.stack([pick([-1.0, 0.5, 1.0, 2.0], c), pick([-0.5, 0.25, 0.5, 1.0], c),
                                   torch.randint(-8, 9, (c,), generator=g).float() / 4]))
        d['shift'] = d['shift'] - 0.25 * (d['scale'] == 0.5)       # y / 2 is a half-integer too: an odd quarter keeps z off 0
    else:
        d = dict(y=bf(r(m, c) * 1.5 + 0.3), shortcut=bf(r(m, c)), dout=bf(r(m, c)), ds0=bf(r(m, c)),
                 scale=0.5 + 1.5 * torch.rand(c, generator=g), shift=0.5 * r(c), mean=0.3 + 0.3 * r(c),
                 rstd=0.4 + 0.6 * torch.rand(c, generator=g), coef=torch.stack([0.5 + r(c).abs(), 0.1 * r(c), 0.01 * r(c)]))
    return {k: v.contiguous() for k, v in d.items()}


class StreamRef:
    """fp64 of tok_bn_act_fwd and, per ReLU pattern, of tok_bn_bwd_reduce / tok_bn_bwd_apply"""

    def __init__(self, d, relu, with_sc):
        self.d, self.relu, self.with_sc = d, relu, with_sc
        y, sc, sh = d['y'].double(), d['scale'].double(), d['shift'].double()
        s = d['shortcut'].double() if with_sc else torch.zeros_like(y)
        self.z = y * sc + sh + s
        self.m_out = (y * sc).abs() + sh.abs() + s.abs()
        self.out = self.z.clamp_min(0) if relu else self.z
        self.near = (self.z.abs() <= 2 * U32 * self.m_out) if relu else torch.zeros_like(y, dtype=torch.bool)
        self.pattern = self.z > 0                                  # the forward's ReLU pattern
        self.recomputed = (y * sc + sh) > 0                        # what mask == NULL stands for (no shortcut in it)
        self.near_rec = ((y * sc + sh).abs() <= 2 * U32 * ((y * sc).abs() + sh.abs())) if relu else self.near
        self.mask_bytes = pack_bits(self.pattern)
        self.y2 = torch.stack([y.sum(0), (y * y).sum(0)])
        self.m_y2 = torch.stack([y.abs().sum(0), (y * y).sum(0)])

    def bwd(self, use_mask, acc):
        """dz, the two sums with their absolute sums, dy, dshortcut; `loose` = the elements whose pattern may flip"""
        d = self.d
        y, g = d['y'].double(), d['dout'].double()
        on = (self.pattern if use_mask else self.recomputed) if self.relu else torch.ones_like(y, dtype=torch.bool)
        loose = (self.near_rec if self.relu and not use_mask else torch.zeros_like(on))
        dz = g * on
        xh = (y - d['mean'].double()) * d['rstd'].double()
        c1, c2, c3 = d['coef'].double()
        r = dict(dz=dz, loose=loose, sums=torch.stack([dz.sum(0), (dz * xh).sum(0)]),
                 m_sums=torch.stack([dz.abs().sum(0), (dz * xh).abs().sum(0)]),
                 x_sums=torch.stack([(g.abs() * loose).sum(0), ((g * xh).abs() * loose).sum(0)]),
                 dy=c1 * dz + c2 * y + c3, m_dy=(c1 * dz).abs() + (c2 * y).abs() + c3.abs())
        r['ds'] = dz + d['ds0'].double() if acc else dz
        r['m_ds'] = dz.abs() + d['ds0'].double().abs() if acc else torch.zeros_like(dz)
        return r


def assert_exact_sums(ref, b):
    """the integer run: every sum stays below 2^24 units of the last place of its terms (1 for dz and y, 1/2 for dz xhat, 1/4 for out)"""
    assert float(ref.m_y2.max()) < 2 ** 24 and float(b['m_sums'][0].max()) < 2 ** 24 and 2 * float(b['m_sums'][1].max()) < 2 ** 24
    assert 4 * float(ref.out.abs().sum(0).max()) < 2 ** 24


def _eq(mine, ref, what):
    mine, ref = mine.detach().double().cpu(), ref.detach().double().cpu()
    assert mine.shape == ref.shape, (what, tuple(mine.shape), tuple(ref.shape))
    bad = mine != ref
    if bool(bad.any()):
        i = bad.reshape(-1).nonzero()[0, 0]
        idx = tuple(int(v) for v in torch.unravel_index(i, bad.shape))
        raise AssertionError(f'{what}: {int(bad.sum())} elements differ from fp64, first {idx}: {float(mine.reshape(-1)[i])!r} != '
                             f'{float(ref.reshape(-1)[i])!r}')


def _near_ok(near, what):
    share = float(near.double().mean())
    assert share <= NEAR_SHARE, f'{what}: {share:.2e} of the elements lie within the fp32 error of z = 0'


def check_out(tag, ref, out, integer, frac=1.0):
    if integer:
        return _eq(out, ref.out, 'out')
    _near_ok(ref.near, 'out')
    keep = ~ref.near
    assert_bounded(out[keep], ref.out[keep], ref.m_out[keep], A_BF if frac == 1.0 else 0.0, frac * B_OUT, 'out', tag if frac == 1.0 else None)


def check_mask(ref, out, mask_bits):
    """mask bit = (the kernel's own stored out > 0), and the fp64 pattern outside the near band"""
    assert torch.equal(mask_bits, out.float() > 0), 'mask bits differ from (out > 0)'
    if ref.relu:
        keep = ~ref.near
        assert torch.equal(mask_bits[keep], ref.pattern[keep]), 'mask bits differ from the fp64 ReLU pattern'


def check_sums(tag, what, mine, ref, mag, extra, n, integer, frac=1.0):
    """mine: the partial rows folded in fp64, [2][c]"""
    if integer:
        return _eq(mine, ref, what)
    for i, name in enumerate(('s1', 's2')):
        assert_bounded(mine[i], ref[i], frac * n * U32 * mag[i] + extra[i], 0.0, 1.0, f'{what}_{name}', tag if frac == 1.0 else None)


def check_colsum(tag, out_mine, folded, m, c, integer, ref=None, frac=1.0):
    o = out_mine.double()
    if integer:
        return _eq(folded, ref.out.sum(0), 'colsum')
    assert_bounded(folded, o.sum(0), o.abs().sum(0), 0.0, frac * (n_sum(m, c) - 3) * U32, 'colsum', tag if frac == 1.0 else None)


def check_apply(tag, b, dy, ds, acc, integer, frac=1.0):
    rec = tag if frac == 1.0 else None
    if integer:
        _eq(dy, b['dy'], 'dy')
        if ds is not None:
            _eq(ds, b['ds'], 'dshortcut')
        return
    _near_ok(b['loose'], 'dy')
    keep = ~b['loose']
    assert_bounded(dy[keep], b['dy'][keep], b['m_dy'][keep], A_BF if frac == 1.0 else 0.0, frac * B_DY, 'dy', rec)
    if ds is not None and acc:
        assert_bounded(ds[keep], b['ds'][keep], b['m_ds'][keep], A_BF if frac == 1.0 else 0.0, frac * B_DS, 'dshortcut', rec)
    elif ds is not None:
        _eq(ds[keep], b['ds'][keep], 'dshortcut (a masked copy: exact)')


def kernel_rows(t, m, c):
    """[m][c] -> the terms of each partial row in the kernel's ownership: [trips][rows][rpb][c], zero padded"""
    rpb, rows = geo(c)[2], part_rows(m, c)
    trips = cdiv(m, rows * rpb)
    pad = torch.zeros(trips * rows * rpb - m, c, dtype=t.dtype)
    return torch.cat([t, pad]).view(trips, rows, rpb, c)


def fp32_sum(t, m, c):
    """column sums in fp32 in the kernel's partition: per thread over the trips in order, then over the rows of a block, the
    partial rows folded in fp64"""
    k = kernel_rows(t.float(), m, c)
    acc = torch.zeros_like(k[0])
    for i in range(k.shape[0]):
        acc = acc + k[i]
    return acc.sum(1).double().sum(0)


def fp32_stream(d, relu, with_sc, use_mask, acc, pattern):
    """the kernels' formulas in plain fp32 torch, unfused, before the bf16 stores.  `pattern`: the mask handed to the backward"""
    y, sc, sh = d['y'].float(), d['scale'], d['shift']
    m, c = y.shape
    z = y * sc + sh
    zr = z
    if with_sc:
        z = z + d['shortcut'].float()
    out = z.clamp_min(0) if relu else z
    on = (pattern if use_mask else zr > 0) if relu else torch.ones_like(y, dtype=torch.bool)
    dz = d['dout'].float() * on
    xh = (y - d['mean']) * d['rstd']
    sums = torch.stack([fp32_sum(dz, m, c), fp32_sum(dz * xh, m, c)])
    stats = torch.stack([fp32_sum(y, m, c), fp32_sum(y * y, m, c)])
    c1, c2, c3 = d['coef']
    dy = c1 * dz + c2 * y + c3
    ds = dz + d['ds0'].float() if acc else dz
    return dict(out=out, sums=sums, stats=stats, dy=dy, ds=ds, colsum=fp32_sum(bf(out), m, c))


# ---- finalize kernels ----------------------------------------------------------------------------------------------------
def finalize_rows(rows, c, integer, seed=0):
    """partial rows [2][rows][c] (fp32), count, and per-channel parameters.  Real: channel 0 has mean 64 / std 0.5, channel 1 is
    constant 3 (variance 0: its rows are exact), the others mean ~0.3 / std ~1.5; every row stands for `per` elements."""
    g = torch.Generator().manual_seed(seed * 104729 + rows * 131 + c)
    if integer:
        count = 256
        s1 = torch.randint(1, 4, (rows, c), generator=g).float() * (2 * torch.randint(0, 2, (rows, c), generator=g).float() - 1)
        s2 = torch.randint(40, 61, (rows, c), generator=g).float() * (1 + rows // 8)       # var = S2 / n - mu^2 > 0
        stats = torch.stack([s1, s2])
    else:
        per = 32
        count = per * rows
        y = torch.randn(rows, per, c, generator=g) * 1.5 + 0.3
        y[..., 0] = 64.0 + 0.5 * torch.randn(rows, per, generator=g)
        y = bf(y).double()
        y[..., 1] = 3.0
        stats = torch.stack([y.sum(1), (y * y).sum(1)]).float()
    p = dict(stats=stats.contiguous(), count=count, gamma=1.0 + 0.3 * torch.randn(c, generator=g), beta=0.3 * torch.randn(c, generator=g),
             rm=0.2 * torch.randn(c, generator=g), rv=0.5 + torch.rand(c, generator=g))
    return p


class FinalizeRef:
    """fp64 of tok_bn_finalize from the same fp32 rows; c_real <= c: the pad channels are 0"""

    def __init__(self, p, c_real=None, count=None):
        st = p['stats'].double()
        rows, c = st.shape[1], st.shape[2]
        cr = c if c_real is None else c_real
        n = p['count'] if count is None else count
        mom = float(torch.tensor(MOMENTUM, dtype=torch.float32))        # the fp32 value the kernel is handed
        S = st.sum(1)[:, :cr]
        g, b = p['gamma'].double()[:cr], p['beta'].double()[:cr]
        mu = S[0] / n
        m2 = S[1].abs() / n + mu * mu
        var = (S[1] / n - mu * mu).clamp_min(0)
        e_var = (rows + 4) * 2.0 ** -52 * m2
        unb = n / (n - 1) if n > 1 else 1.0
        rstd = (var + EPS) ** -0.5
        scale = g * rstd
        pad = lambda t: torch.cat([t, torch.zeros(c - cr, dtype=F64)])      # noqa: E731
        self.c, self.cr, self.var, self.S = c, cr, var, S
        self.mean, self.b_mean = pad(mu), pad(2 * U32 * mu.abs())
        b_rstd = rstd * (8 * U32 + 0.5 * e_var / (var + EPS))
        self.rstd, self.b_rstd = pad(rstd), pad(b_rstd)
        b_scale = g.abs() * b_rstd + 2 * U32 * scale.abs()
        self.scale, self.b_scale = pad(scale), pad(b_scale)
        self.shift = pad(b - mu * scale)
        self.b_shift = pad(mu.abs() * b_scale + scale.abs() * self.b_mean[:cr] + 4 * U32 * ((mu * scale).abs() + b.abs()))
        rm, rv = p['rm'].double()[:cr], p['rv'].double()[:cr]
        self.rm = mom * mu + (1 - mom) * rm
        self.b_rm = mom * self.b_mean[:cr] + 8 * U32 * ((mom * mu).abs() + ((1 - mom) * rm).abs())
        self.rv = mom * var * unb + (1 - mom) * rv
        self.b_rv = mom * unb * e_var + 8 * U32 * (mom * unb * var + ((1 - mom) * rv).abs())

    def check(self, tag, mean, rstd, scale, shift, rm=None, rv=None, frac=1.0):
        rec = tag if frac == 1.0 else None
        for name, mine in (('mean', mean), ('rstd', rstd), ('scale', scale), ('shift', shift)):
            assert_bounded(mine, getattr(self, name), getattr(self, 'b_' + name), 0.0, frac, name, rec)
            assert bool((mine[self.cr:] == 0).all()), f'{name}: pad channels are not zero'
        if rm is not None:
            assert_bounded(rm, self.rm, self.b_rm, 0.0, frac, 'running_mean', rec)
            assert_bounded(rv, self.rv, self.b_rv, 0.0, frac, 'running_var', rec)


def fp32_finalize(p, count=None):
    """fp64 fold, then everything in plain fp32"""
    n = p['count'] if count is None else count
    S = p['stats'].double().sum(1)
    mu64 = S[0] / n
    var64 = (S[1] / n - mu64 * mu64).clamp_min(0)
    mu, var = mu64.float(), var64.float()
    rstd = 1.0 / torch.sqrt(var + EPS)
    scale = p['gamma'] * rstd
    mom = torch.tensor(MOMENTUM)
    unb = n / (n - 1) if n > 1 else 1.0
    return mu, rstd, scale, p['beta'] - mu * scale, (1 - mom) * p['rm'] + mom * mu, (1 - mom) * p['rv'] + mom * (var64 * unb).float()


def bwd_rows(rows, c, integer, seed=0):
    """partial rows [2][rows][c] of sum(dz), sum(dz * xhat) (or sum(dz * y)), m, gamma / mean / rstd, and a prefill of dgamma / dbeta"""
    g = torch.Generator().manual_seed(seed * 15485863 + rows * 257 + c)
    sign = lambda: 2 * torch.randint(0, 2, (rows, c), generator=g).float() - 1        # noqa: E731
    if integer:
        part = torch.stack([torch.randint(1, 6, (rows, c), generator=g).float() * sign(),
                            torch.randint(1, 9, (rows, c), generator=g).float() * sign()])
        m = 1024
        pre = torch.randint(-9, 10, (2, c), generator=g).float()
        mean, rstd = torch.randint(-2, 3, (c,), generator=g).float(), torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c,), generator=g)]
    else:
        part = torch.randn(2, rows, c, generator=g) * 3.0
        m = 37 * rows
        pre = torch.randn(2, c, generator=g)
        mean, rstd = 0.3 + 0.3 * torch.randn(c, generator=g), 0.4 + 0.6 * torch.rand(c, generator=g)
    return dict(part=part.contiguous(), m=m, gamma=1.0 + 0.3 * torch.randn(c, generator=g), mean=mean, rstd=rstd.contiguous(), pre=pre)


class BwdFinalizeRef:
    def __init__(self, p, dzy_form=0, accumulate=0, c_real=None):
        part = p['part'].double()
        rows, c = part.shape[1], part.shape[2]
        cr = c if c_real is None else c_real
        S = part.sum(1)[:, :cr]
        A = part.abs().sum(1)[:, :cr]
        g, mu, rs = p['gamma'].double()[:cr], p['mean'].double()[:cr], p['rstd'].double()[:cr]
        m = p['m']
        s1, s2, e_s2 = S[0], S[1], torch.zeros(cr, dtype=F64)
        if dzy_form:
            s2 = rs * (S[1] - mu * S[0])
            e_s2 = (rows + 4) * 2.0 ** -52 * rs * (A[1] + mu.abs() * A[0])
        pre = p['pre'].double()[:, :cr] if accumulate else torch.zeros(2, cr, dtype=F64)
        self.cr = cr
        self.dgamma, self.dbeta = s2 + pre[0], s1 + pre[1]
        self.b_dgamma = 2 * U32 * s2.abs() + e_s2 + (2 * U32 * (pre[0].abs() + s2.abs()) if accumulate else 0)
        self.b_dbeta = 2 * U32 * s1.abs() + (2 * U32 * (pre[1].abs() + s1.abs()) if accumulate else 0)
        c1 = g * rs
        c2 = -c1 * rs * (s2 / m)
        c3 = -c1 * (s1 / m) - c2 * mu
        b_c2 = 8 * U32 * c2.abs() + (c1 * rs).abs() * e_s2 / m
        pad = lambda t: torch.cat([t, torch.zeros(c - cr, dtype=F64)])      # noqa: E731
        self.coef = torch.stack([pad(c1), pad(c2), pad(c3)])
        self.b_coef = torch.stack([pad(2 * U32 * c1.abs()), pad(b_c2), pad(mu.abs() * b_c2 + 8 * U32 * ((c2 * mu).abs() + (c1 * s1 / m).abs()))])

    def check(self, tag, coef, dgamma=None, dbeta=None, exact_sums=False, frac=1.0):
        rec = tag if frac == 1.0 else None
        assert_bounded(coef, self.coef, self.b_coef, 0.0, frac, 'coef', rec)
        assert bool((coef[:, self.cr:] == 0).all()), 'coef: pad channels are not zero'
        for name, mine in (('dgamma', dgamma), ('dbeta', dbeta)):
            if mine is None:
                continue
            if exact_sums:
                _eq(mine, getattr(self, name), name)
            else:
                assert_bounded(mine, getattr(self, name), getattr(self, 'b_' + name), 0.0, frac, name, rec)


def fp32_bwd_finalize(p, dzy_form, accumulate):
    S = p['part'].double().sum(1)
    mu, rs, g = p['mean'], p['rstd'], p['gamma']
    s2 = rs.double() * (S[1] - mu.double() * S[0]) if dzy_form else S[1]
    sdz, sdzx = S[0].float(), s2.float()
    m1, m2 = (S[0] / p['m']).float(), (s2 / p['m']).float()
    c1 = g * rs
    c2 = -c1 * rs * m2
    coef = torch.stack([c1, c2, -c1 * m1 - c2 * mu])
    return coef, (p['pre'][0] + sdzx if accumulate else sdzx), (p['pre'][1] + sdz if accumulate else sdz)


# ---- the chain on the device's own intermediates --------------------------------------------------------------------------
class ChainRef:
    """tok_bn_stats -> tok_bn_finalize -> act_fwd -> bwd_reduce -> bwd_finalize -> bwd_apply against fp64 training BatchNorm
    (+ shortcut, ReLU) and its gradient.  The element bounds are those of out / dy plus the propagated error of the
    statistics: with N = n_sum(m, c) the fp32 column sums carry e_mu = N u32 mean|y| and e_var = N u32 mean(y^2) + 2 |mu| e_mu,
    rstd / scale / shift follow FinalizeRef's formulas with this e_var, xhat moves by rstd e_mu + |y - mu| b_rstd, the backward
    sums by N u32 sum|term| + sum|dz| e_xhat, and c1, c2, c3 by the formulas of BwdFinalizeRef with these sum errors."""

    def __init__(self, y, shortcut, dout, gamma, beta):
        m, c = y.shape
        N = n_sum(m, c) * U32
        yd, g, b = y.double(), gamma.double(), beta.double()
        s = shortcut.double()
        mu = yd.mean(0)
        var = ((yd - mu) ** 2).mean(0)
        rstd = (var + EPS) ** -0.5
        scale, shift = g * rstd, b - mu * g * rstd
        e_mu = N * yd.abs().mean(0) + 2 * U32 * mu.abs()
        e_var = N * (yd * yd).mean(0) + 2 * mu.abs() * e_mu
        b_rstd = rstd * (8 * U32 + 0.5 * e_var / (var + EPS))
        b_scale = g.abs() * b_rstd + 2 * U32 * scale.abs()
        b_shift = mu.abs() * b_scale + scale.abs() * e_mu + 4 * U32 * ((mu * scale).abs() + b.abs())
        z = yd * scale + shift + s
        self.out = z.clamp_min(0)
        self.m_out = (yd * scale).abs() + shift.abs() + s.abs()
        self.e_out = yd.abs() * b_scale + b_shift                              # added to the element bound of out
        self.near = z.abs() <= 2 * U32 * self.m_out + self.e_out
        dz = dout.double() * (z > 0)
        xh = (yd - mu) * rstd
        e_xh = rstd * e_mu + (yd - mu).abs() * b_rstd
        loose = dout.double().abs() * self.near
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
        self.stats = (mu, rstd, b_rstd, e_mu)

    def check(self, tag, out, dy, frac=1.0):
        _near_ok(self.near, 'chain')
        k = ~self.near
        a = A_BF if frac == 1.0 else 0.0
        rec = tag if frac == 1.0 else None
        assert_bounded(out[k], self.out[k], (frac * B_OUT * self.m_out + (1 + a) * self.e_out)[k], a, 1.0, 'out', rec)
        assert_bounded(dy[k], self.dy[k], (frac * B_DY * self.m_dy + (1 + a) * self.e_dy)[k], a, 1.0, 'dy', rec)


# ---- fused stem -----------------------------------------------------------------------------------------------------------
def stem_inputs(n, h, w, c, integer, seed=0):
    p, q = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    d = stream_inputs(n * h * w, c, integer, seed + 5)
    g = torch.Generator().manual_seed(seed + n * h * w + c)
    d['dpool'] = torch.randint(-4, 5, (n * p * q, c), generator=g).to(BF) if integer else bf(torch.randn(n * p * q, c, generator=g))
    d['dims'] = (n, h, w, c, p, q)
    return d


def _taps(n, h, w, p, q):
    """per tap t = 3 r + s: (valid [p][q], flat position index [p][q]) of window (p, q)"""
    pp, qq = torch.arange(p).view(p, 1), torch.arange(q).view(1, q)
    for t in range(9):
        hh, ww = 2 * pp - 1 + t // 3, 2 * qq - 1 + t % 3
        ok = (hh >= 0) & (hh < h) & (ww >= 0) & (ww < w)
        yield t, ok.expand(p, q), (hh.clamp(0, h - 1) * w + ww.clamp(0, w - 1)).expand(p, q)


class StemRef:
    """independent fp64 reference: z = relu(y scale + shift); 3x3 / stride 2 / pad 1 max, the first maximum in (r, s) scan order;
    the gradient of each pooled element goes to its tap; then the BatchNorm sums and apply on d(z) = gathered gradient * (z > 0)"""

    def __init__(self, d):
        n, h, w, c, p, q = self.dims = d['dims']
        y = d['y'].double().view(n, h * w, c)
        sc, sh = d['scale'].double(), d['shift'].double()
        zr = y * sc + sh
        z = zr.clamp_min(0)
        mag = (y * sc).abs() + sh.abs()
        self.z, self.mag, self.on = z, mag, zr > 0
        self.near = zr.abs() <= 2 * U32 * mag
        best = torch.full((n, p, q, c), -float('inf'), dtype=F64)
        tap = torch.zeros((n, p, q, c), dtype=torch.long)
        bmag = torch.zeros((n, p, q, c), dtype=F64)
        for t, ok, flat in _taps(n, h, w, p, q):
            v = z[:, flat.reshape(-1)].view(n, p, q, c)
            better = ok[None, :, :, None] & (v > best)
            best = torch.where(better, v, best)
            tap = torch.where(better, torch.full_like(tap, t), tap)
            bmag = torch.maximum(bmag, torch.where(ok[None, :, :, None], mag[:, flat.reshape(-1)].view(n, p, q, c), bmag))
        self.pooled, self.tap, self.m_pooled = best, tap, bmag
        self.ypool = self.gather(d['y'], tap)

    def flat_of(self, tap):
        n, h, w, c, p, q = self.dims
        pp, qq = torch.arange(p).view(1, p, 1, 1), torch.arange(q).view(1, 1, q, 1)
        return (2 * pp - 1 + tap // 3) * w + (2 * qq - 1 + tap % 3)

    def gather(self, t, tap):
        """t [n h w][c] at the position each window's tap names -> [n][p][q][c]"""
        n, h, w, c, p, q = self.dims
        return torch.gather(t.view(n, h * w, c), 1, self.flat_of(tap).view(n, p * q, c)).view(n, p, q, c)

    def bwd(self, d, tap):
        """with the tap indices the backward kernels are handed"""
        n, h, w, c, p, q = self.dims
        idx = self.flat_of(tap.long()).view(n, p * q, c)
        gp = d['dpool'].double().view(n, p * q, c)
        z0 = torch.zeros(n, h * w, c, dtype=F64)
        g = z0.clone().scatter_add_(1, idx, gp)
        gabs = z0.clone().scatter_add_(1, idx, gp.abs())
        cnt = z0.clone().scatter_add_(1, idx, torch.ones_like(gp))
        e_g = torch.where(cnt >= 2, A_BF * g.abs() + 6 * U32 * gabs, z0) * self.on
        y = d['y'].double().view(n, h * w, c)
        dz = g * self.on
        xh = (y - d['mean'].double()) * d['rstd'].double()
        c1, c2, c3 = d['coef'].double()
        loose = self.near
        f = lambda t: t.reshape(n * h * w, c)             # noqa: E731
        return dict(dz=f(dz), loose=f(loose), e_g=f(e_g), sums=torch.stack([f(dz).sum(0), f(dz * xh).sum(0)]),
                    m_sums=torch.stack([f(dz).abs().sum(0), f(dz * xh).abs().sum(0)]),
                    x_sums=torch.stack([f(e_g + gabs * loose).sum(0), f((e_g + gabs * loose) * xh.abs()).sum(0)]),
                    dy=f(c1 * dz + c2 * y + c3), m_dy=f((c1 * dz).abs() + (c2 * y).abs() + c3.abs()), e_dy=f(c1.abs() * e_g))

    def pooled_sums(self, d, pooled, ypool):
        """tok_bn_pool_bwd_reduce_pooled's own contract on the tensors it is handed: over pooled elements with pooled > 0"""
        c = self.dims[3]
        gz = d['dpool'].double().view(-1, c) * (pooled.double().view(-1, c) > 0)
        xh = (ypool.double().view(-1, c) - d['mean'].double()) * d['rstd'].double()
        return torch.stack([gz.sum(0), (gz * xh).sum(0)]), torch.stack([gz.abs().sum(0), (gz * xh).abs().sum(0)])


def check_stem_fwd(tag, d, ref, pooled, argmax, ypool, integer, frac=1.0):
    n, h, w, c, p, q = d['dims']
    tap = argmax.long().view(n, p, q, c)
    pooled = pooled.view(n, p, q, c)
    for t, ok, _ in _taps(n, h, w, p, q):
        assert not bool(((tap == t) & ~ok[None, :, :, None]).any()), f'argmax names tap {t} outside the map'
    assert int(tap.max()) <= 8
    if ypool is not None:
        assert torch.equal(ypool.view(n, p, q, c), ref.gather(d['y'], tap)), 'ypool is not the raw y at the named tap'
    if integer:
        _eq(pooled, ref.pooled, 'pooled')
        assert torch.equal(tap, ref.tap), 'argmax: ties go to the first tap in (r, s) scan order'
        return
    a = A_BF if frac == 1.0 else 0.0
    rec = tag if frac == 1.0 else None
    assert_bounded(pooled, ref.pooled, ref.m_pooled, a, frac * B_OUT, 'pooled', rec)
    at_tap = ref.gather(ref.z.reshape(-1, c), tap)
    assert_bounded(pooled, at_tap, ref.gather(ref.mag.reshape(-1, c), tap), a, frac * B_OUT, 'pooled_vs_named_tap', rec)


def check_stem_bwd(tag, b, m, c, folded, dy, integer, frac=1.0):
    if integer:
        _eq(folded, b['sums'], 'pool_reduce')
        return _eq(dy, b['dy'], 'pool_dy')
    _near_ok(b['loose'], 'stem')
    check_sums(tag, 'pool_reduce', folded, b['sums'], b['m_sums'], b['x_sums'], n_sum(m, c), False, frac)
    k = ~b['loose']
    a = A_BF if frac == 1.0 else 0.0
    assert_bounded(dy[k], b['dy'][k], (frac * B_DY * b['m_dy'] + (1 + a) * b['e_dy'])[k], a, 1.0, 'pool_dy', tag if frac == 1.0 else None)


def fp32_stem(d, ref):
    """plain fp32: forward on unrounded z (the reference's taps handed to the backward), d(z) rounded to bf16 where windows meet"""
    n, h, w, c, p, q = d['dims']
    y = d['y'].float()
    zr = y * d['scale'] + d['shift']
    z = zr.clamp_min(0).view(n, h * w, c)
    best = torch.full((n, p, q, c), -float('inf'))
    tap = torch.zeros((n, p, q, c), dtype=torch.long)
    for t, ok, flat in _taps(n, h, w, p, q):
        v = z[:, flat.reshape(-1)].view(n, p, q, c)
        better = ok[None, :, :, None] & (v > best)
        best, tap = torch.where(better, v, best), torch.where(better, torch.full_like(tap, t), tap)
    idx = ref.flat_of(ref.tap).view(n, p * q, c)
    g = torch.zeros(n, h * w, c).scatter_add_(1, idx, d['dpool'].float().view(n, p * q, c))
    dz = bf(g).float().view(n * h * w, c) * (zr > 0)
    xh = (y - d['mean']) * d['rstd']
    m = n * h * w
    c1, c2, c3 = d['coef']
    return best, tap, torch.stack([fp32_sum(dz, m, c), fp32_sum(dz * xh, m, c)]), c1 * dz + c2 * y + c3
