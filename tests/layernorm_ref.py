"""fp64 reference of tok_layernorm_fwd / _bwd (include/tok.h) on the same bf16 inputs, the bounds of the contract and a plain
fp32 run of the same formulas (tests/test_layernorm_ref.py: it stays inside half of every bound).

  out    |err| <= 2^-8 |ref| + 2^-16 mag,  mag = ((|x| + |mu|) rstd |gamma| + |beta|) |row_scale| + |shortcut|
         (one bf16 rounding; the fp32 sums are eight sequential adds and a lane tree: 2^-16 is about 8x over that)
  mean   |err| <= 2^-16 mean|x|
  rstd   |err| <= rstd (1/2 (2^-16 var + dmu^2) / (var + eps) + 2^-20),  dmu = 2^-16 mean|x|: the condition number of the variance
         times the error of a TWO-PASS variance (mean((x - mu')^2) = var + (mu' - mu)^2 exactly, the first-order term vanishes;
         a one-pass E[x^2] - mu^2 on rows with a common offset does not pass), plus 16 ulp for the reciprocal square root
  dx     |err| <= 2^-8 |ref| + 2^-16 rstd (|g| + mean|g| + |xh| mean|g xh|),  g = dout row_scale gamma; the backward is fed the
         fp32-rounded fp64 statistics, so it is tested alone; ref includes the previous dx under accumulate
  dgamma, dbeta   the fp64 fold of the partial rows: |err| <= 2^-16 sum|dout row_scale xh|, 2^-16 sum|dout row_scale|"""
import torch

from helpers import A_BF, assert_bounded

EPS = 1e-5
B_LN = 2.0 ** -16


def make_inputs(rows, c, shortcut, row_scale, seed):
    """x, dout, dx0, shortcut (bf16), gamma, beta, row_scale (fp32), rows_per_sample.  From five rows on: row 0 is constant
    (variance 0), row 1 is 64 + 0.5 noise, row 2 is zero.  row_scale has a 0 for its second sample."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, c, generator=g) * 2.0 + 0.5
    if rows >= 5:
        x[0] = 3.0
        x[1] = 64.0 + 0.5 * torch.randn(c, generator=g)
        x[2] = 0.0
    bf = lambda t: t.to(torch.bfloat16)          # noqa: E731
    dout, dx0 = torch.randn(rows, c, generator=g), torch.randn(rows, c, generator=g)
    sh = bf(torch.randn(rows, c, generator=g)) if shortcut else None
    gamma, beta = 1.0 + 0.3 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)
    rps, scale = rows, None
    if row_scale:
        rps = max(1, -(-rows // 3))
        scale = torch.tensor([1.5, 0.0, 0.7, 1.0, 2.0])[:-(-rows // rps)].clone()
    return dict(x=bf(x), dout=bf(dout), dx0=bf(dx0), shortcut=sh, gamma=gamma, beta=beta, row_scale=scale, rps=rps)


class LNRef:
    def __init__(self, d):
        x, gamma, beta = d['x'].double(), d['gamma'].double(), d['beta'].double()
        rows, c = x.shape
        sc = torch.ones(rows, 1, dtype=torch.float64) if d['row_scale'] is None else \
            d['row_scale'].double().repeat_interleave(d['rps'])[:rows, None]
        sh = torch.zeros(rows, c, dtype=torch.float64) if d['shortcut'] is None else d['shortcut'].double()
        self.sc, self.sh = sc, sh
        mu = x.mean(1, keepdim=True)
        var = ((x - mu) ** 2).mean(1, keepdim=True)
        rstd = (var + EPS) ** -0.5
        self.mean, self.rstd = mu[:, 0], rstd[:, 0]
        self.out = ((x - mu) * rstd * gamma + beta) * sc + sh
        self.m_out = ((x.abs() + mu.abs()) * rstd * gamma.abs() + beta.abs()) * sc.abs() + sh.abs()
        self.m_mean = x.abs().mean(1)
        dmu = B_LN * self.m_mean
        self.b_rstd = self.rstd * (0.5 * (B_LN * var[:, 0] + dmu ** 2) / (var[:, 0] + EPS) + 2.0 ** -20)
        # backward on the statistics the kernel is given
        self.mean32, self.rstd32 = self.mean.float(), self.rstd.float()
        m, r = self.mean32.double()[:, None], self.rstd32.double()[:, None]
        go = d['dout'].double() * sc
        xh = (x - m) * r
        g = go * gamma
        self.dx = [r * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))]
        self.dx.append(self.dx[0] + d['dx0'].double())
        self.m_dx = r * (g.abs() + g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True))
        self.dgamma, self.dbeta = (go * xh).sum(0), go.sum(0)
        self.m_dgamma, self.m_dbeta = (go * xh).abs().sum(0), go.abs().sum(0)


def check_fwd(tag, ref, out, mean, rstd, frac=1.0):
    """frac < 1: for UNROUNDED fp32 results (the bf16 rounding term, which a rounding may use up entirely, is left out)"""
    rec = tag if frac == 1.0 else None
    assert_bounded(out, ref.out, ref.m_out, A_BF if frac == 1.0 else 0.0, frac * B_LN, 'out', rec)
    assert_bounded(mean, ref.mean, ref.m_mean, 0.0, frac * B_LN, 'mean', rec)
    assert_bounded(rstd, ref.rstd, ref.b_rstd, 0.0, frac, 'rstd', rec)


def check_bwd(tag, ref, acc, dx, dgamma, dbeta, frac=1.0):
    rec = f'{tag}_acc{acc}' if frac == 1.0 else None
    assert_bounded(dx, ref.dx[acc], ref.m_dx, A_BF if frac == 1.0 else 0.0, frac * B_LN, 'dx', rec)
    assert_bounded(dgamma, ref.dgamma, ref.m_dgamma, 0.0, frac * B_LN, 'dgamma', rec)
    assert_bounded(dbeta, ref.dbeta, ref.m_dbeta, 0.0, frac * B_LN, 'dbeta', rec)


def fp32_run(d, ref, acc):
    """the same formulas in fp32 (torch's summation order), before the bf16 rounding of out and dx"""
    x, gamma, beta = d['x'].float(), d['gamma'], d['beta']
    rows, c = x.shape
    sc = torch.ones(rows, 1) if d['row_scale'] is None else d['row_scale'].repeat_interleave(d['rps'])[:rows, None]
    mu = x.sum(1, keepdim=True) / c
    var = ((x - mu) ** 2).sum(1, keepdim=True) / c
    rstd = torch.rsqrt(var + EPS)
    out = ((x - mu) * rstd * gamma + beta) * sc
    if d['shortcut'] is not None:
        out = out + d['shortcut'].float()
    m, r = ref.mean32[:, None], ref.rstd32[:, None]
    go = d['dout'].float() * sc
    xh = (x - m) * r
    g = go * gamma
    dx = r * (g - g.sum(1, keepdim=True) / c - xh * ((g * xh).sum(1, keepdim=True) / c))
    if acc:
        dx = dx + d['dx0'].float()
    return out, mu[:, 0], rstd[:, 0], dx, (go * xh).sum(0), go.sum(0)
