"""fp64 references of the fused residual unit's host-free kernels (csrc/unit3.hip: tok_bn_gram_finalize, tok_bn3_bwd_prepare) and of
the gradient-clip kernels (csrc/grad_clip.hip: tok_grad_sqnorm_partial, tok_grad_clip_coef, tok_grad_scale, tok_grad_clamp), the
bounds of their contracts, the input makers and the case lists (tests/test_unit3_clip_ref.py holds them to torch: fp64 autograd of
relu(batch_norm(z Wq^T) + shortcut), torch.nn.utils.clip_grad_norm_ / clip_grad_value_; wrong restatements do not pass).
Plain torch / numpy, no HIP.

Every reference is computed from EXACTLY the operands the kernel receives (the fp32 Z, zsum, G, wz, partial rows, mean, rstd; never
from z), so a comparison has only the kernel's own roundings in it.  Every check is |mine - ref| <= bound per element.
U32 = 2^-24 (fp32 unit roundoff), U64 = 2^-53, A_BF = 2^-8 (one bf16 rounding).  A product of two fp32 values is exact in fp64.

tok_bn_gram_finalize (wq = bf16(w), M = count, mu = zsum / M):
  mean     fp64 fold of P exact products, one division, one cast:                 U32 |mean| + (P + 4) U64 sum |wq| |zsum| / M
  wz       T = wq Z, an fp32 fma chain of P terms (any split into slices):        (P + 1) U32 |wq| |Z|
  var      BLOCK path (P in {64, 128, 256}): the centred row sum_q wq_q (Z[q][p] - zsum_q zsum_p / M) in fp64, times wq_p, folded in
           fp64, over M:     dvar = 4 (P + 4) U64 |wq|^T (|Z| + |zsum| |zsum|^T / M) |wq| / M     (fp64 ulps of the UNcentred magnitude)
           GENERIC path (any other P): var = <T_k, wq_k> / M - mean^2 in fp64 from the fp32 T, so T's chain is in it:
                 dvar += (P + 2) U32 |wq|^T |Z| |wq| / M        (`uncentred_bound`)
           This is a worst-case bound of a difference that cancels: small against the value on the plain inputs, but on the
           large-mean input (mean 2, std 0.05) 0.24 of the value at P = 72 and larger than the value at P = 320.  There the generic
           path's rstd is bounded by measurement instead (`large_mean_rstd`: 4 x the largest deviation of the same formula in the
           kernel's order on the CPU, about 1e-3 and 2e-3 of the value), beside the 5e-2 norm ratio against the true variance that
           the block path has to meet.
  rstd     1 / sqrt(var + eps) is monotone, so dvar is carried through exactly: the worse of the two ends of
           [1 / sqrt(var + dvar + eps), 1 / sqrt(max(var - dvar, 0) + eps)], plus the cast: + 2 U32 rstd.  (For dvar << var + eps this
           is the derivative bound rstd^3 dvar / 2; the interval form also holds where var = 0.)
  scale    fl32(gamma rstd):   |gamma| b_rstd + U32 |scale|
  shift    fma(-mean, scale, beta), one rounding:   |mean| b_scale + (|scale| + b_scale) b_mean + U32 (|shift| + those)
  running  (1 - mom) r + mom s in fp32, 4 roundings at most:   4 U32 (|(1 - mom) r| + |mom s|) + mom b_s;  s = mean, or var * unbias
           with b = unbias (dvar + U32 var)
tok_bn3_bwd_prepare (a1 = sum of the partial rows, a2 = <G_k, wq_k>, sx = rstd (a2 - mean a1)):
  dbeta    fp64 fold of `rows` fp32 values (exact products none), one cast:       U32 |a1| + (rows + 2) U64 sum |partial|
  dgamma   U32 |sx| + (P + rows + 6) U64 rstd (sum |G wq| + |mean| sum |partial|)
           accumulate adds one fp32 addition: + U32 |prior + value|
  coef     c1 = fl32(gamma rstd): U32 |c1|;   c2 = -c1 rstd fl32(sx / M): 4 U32 |c2| (+ the fp64 term of sx);
           c3 = -c1 fl32(a1 / M) - c2 mean:   4 U32 |c1 m1| + 6 U32 |c2 mean|   (absolute: the two terms cancel)
  dw       fma(c1, G, fma(c2, T, c3 zsum)) (+ prior):   |G| b_c1 + |T| b_c2 + |zsum| b_c3 + 3 U32 (|c1 G| + |c2 T| + |c3 zsum|)
           (+ U32 (|prior| + |value|))
  wa       bf16(fl32(c1 wq)), stored [p][k]:   (A_BF + 3 U32) |ref|
  wb       bf16 of an fp32 chain over the K channels of fl32(c2 wq) wq, in any slice order (the split reduction adds its
           slices: at most K / 64 more additions):   A_BF |ref| + (K + K / 64 + 8) U32 |wq|^T diag|c2| |wq|
  cvec     the same chain over c3:   (K + K / 64 + 4) U32 |c3|^T |wq| + b_c3^T |wq|
gradient clip (grid = clamp(ceil(total / 8192), 1, 1024), chunk = ceil(total / grid), block b owns [b chunk, (b + 1) chunk)):
  partial  an fp64 fma chain per thread (at most 4 ceil(len / 1024) + 6 per span the slice meets) and the 6 + 4 additions of the
           block fold:   (chain + 10) U64 sum x^2, with the reference's own pairwise sum (+ 26 U64) in it: a few fp64 ulps
  norm     (float) sqrt(fold of the partials): bit-equal to `clip_coef_f32`, which restates the fold in the kernel's order; against
           the fp64 norm of the data: U32 |norm| (1 + tiny)
  coef     max_norm / (norm + 1e-6f) clamped to 1, in fp32: bit-equal to the restatement
  scale    x * coef in fp32: bit-exact; coef == 1: no store at all
  clamp    bit-exact against torch.clamp_"""
import functools
import math

import numpy as np
import torch

from helpers import A_BF, BF, F32, U32, cdiv
from loss_ref import bounded, flush_record  # noqa: F401  (used by the test modules)

F64 = torch.float64
U64 = 2.0 ** -53
EPS = 1e-5
MOMENTUM = 0.1
UNIT3_P_MAX = 2048
BLOCK_P = (64, 128, 256)
GRAM_BLOCK = [(64, 8), (64, 256), (128, 24), (256, 264)]
GRAM_GENERIC = [(8, 16), (72, 40), (72, 1032), (320, 640), (512, 128), (1024, 16)]
GRAM_CASES = GRAM_BLOCK + GRAM_GENERIC
PREP_CASES = GRAM_CASES + [(9, 8), (2048, 8)]
COUNTS = (1, 2, 5000)
# one row has variance 0 and two rows a rank-one covariance (some channel's variance is as small against E[y^2] as chance has it): with
# the usual eps no bound of the GENERIC path would be small against such a value, so its count = 1 and count = 2 cases run with a
# large eps.  The block path keeps eps = 1e-5 at every count (its bound is fp64 ulps; against eps alone they are CAP_SMALL_COUNT), and
# make_gram_one_count gives both paths a count = 1 case of non-zero variance at eps = 1e-5.
def count_eps(p, count):
    return EPS if is_block(p) or count > 2 else 2.0


ONE_COUNT_CASES = [(64, 8), (128, 24), (8, 16), (72, 40)]
CHAIN_CASES = [(320, 64, 128), (320, 72, 128)]
ROWS_CASES = (1, 3, 64, 65, 256, 257, 512, 513, 1025)
LARGE_P = (64, 72, 256, 320)
LARGE_K = 16
LARGE_M = 200000
# caps on bound / |value| that the CPU tests assert of every input (tests/test_unit3_clip_ref.py)
CAP_ULP = 2.0 ** -21             # fp64 folds cast to fp32: 8 ulps
CAP_F32 = 2.0 ** -6              # fp32 chains, against the tensor's scale (values cross zero)
CAP_SMALL_COUNT = 2.0 ** -18     # block path, count <= 2: fp64 ulps of E[y^2] against eps alone (var is 0 or as small as chance has it)
CAP_CHAIN = 2.0 ** -4            # the chain case: three bf16 roundings of terms that cancel, against the tensor's scale


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f32(x):
    return float(np.float32(x))


def check(tag, what, mine, ref, bound):
    """|mine - ref| <= bound on EVERY element; the worst ratio of (tag, what) is kept for the parity record"""
    return bounded(mine, ref, bound, 0.0, 1.0, what, tag)


def is_block(p):
    return p in BLOCK_P


# ---- launcher rules, restated -------------------------------------------------------------------------------------------------------
def gemm_splits(m, n, l):
    s = min(cdiv(512, cdiv(n, 64) * cdiv(m, 64)), max(l // 64, 1))
    return max(s, 1)


def ws_floats(p, k):
    return k * (p + 1) + gemm_splits(p + 1, p, k) * (p + 1) * p


def split_slices(p, k):
    """(splits, lchunk, number of slices that hold no element) of the (p + 1) x p x k product of the generic prepare path"""
    s = gemm_splits(p + 1, p, k)
    lchunk = cdiv(cdiv(k, s), 16) * 16
    return s, lchunk, sum(1 for z in range(s) if z * lchunk >= k)


def fold_form(rows):
    return 4 if rows <= 256 else 8 if rows <= 512 else 16


# ---- tok_bn_gram_finalize -----------------------------------------------------------------------------------------------------------
def make_gram(p, k, count, seed=0):
    """Z, zsum of `count` rows (a base sample of at most 96 bf16 rows, scaled: count is only a number), w with an all-zero filter
    row, gamma with a zero and a negative, running statistics"""
    g = gen(1000 * p + k + seed)
    nb = min(count, 96)
    zb = (torch.randn(nb, p, generator=g, dtype=F64) + 0.3).to(BF).double()
    s = count / nb
    w = (torch.randn(k, p, generator=g, dtype=F64) * p ** -0.5).float()
    w[1] = 0
    gamma = (torch.randn(k, generator=g, dtype=F64) * 0.3 + 1).float()
    gamma[0], gamma[2] = 0.0, -0.75
    return dict(p=p, k=k, count=count, Z=(s * (zb.t() @ zb)).float(), zsum=(s * zb.sum(0)).float(), w=w, gamma=gamma,
                beta=torch.randn(k, generator=g, dtype=F64).float(), rm=torch.randn(k, generator=g, dtype=F64).float(),
                rv=(torch.rand(k, generator=g, dtype=F64) + 0.5).float())


def make_gram_one_count(p, k, seed=0):
    """count = 1 with operands that belong to no single row: Z = 32 zb^T zb and zsum = colsum(zb) of 32 base rows, so that
    Z - zsum zsum^T = 32^2 cov(zb) and the operand-level variance is NOT zero: the running variance then shows the unbiased factor
    (1 at count = 1), which a true single row (variance 0) cannot"""
    d = make_gram(p, k, 32, seed + 5)
    d['Z'] = (32.0 * d['Z'].double()).float()
    d['count'] = 1
    return d


@functools.lru_cache(maxsize=None)
def make_large_mean(p, k=LARGE_K, m=LARGE_M, mean=2.0):
    """an input with |mean| >> std (bf16 storage of N(mean, 0.05^2)), Z accumulated in fp32 as the weight-gradient launch leaves it;
    `var_true`: the variance of y = z wq^T from the fp64 moments of the same rows"""
    g = gen(p + k)
    Z32, Z64, s64 = torch.zeros(p, p), torch.zeros(p, p, dtype=F64), torch.zeros(p, dtype=F64)
    for _ in range(0, m, 25000):
        z = (torch.randn(25000, p, generator=g) * 0.05 + mean).to(BF).float()
        Z32 += z.t() @ z
        zd = z.double()
        Z64 += zd.t() @ zd
        s64 += zd.sum(0)
    w = (torch.randn(k, p, generator=g, dtype=F64) * p ** -0.5).float()
    wq = w.to(BF).double()
    mu = s64 / m
    var_true = ((wq @ (Z64 / m - torch.outer(mu, mu))) * wq).sum(1)
    return dict(p=p, k=k, count=m, Z=Z32, zsum=s64.float(), w=w, gamma=torch.ones(k), beta=torch.zeros(k), rm=torch.zeros(k),
                rv=torch.ones(k), var_true=var_true)


class Out:
    """a reference value and its bound"""

    def __init__(self, ref, bound):
        self.ref, self.bound = ref, bound

    def __iter__(self):
        return iter((self.ref, self.bound))


def _rstd_bound(var, dvar, eps):
    ref = 1.0 / torch.sqrt(var + eps)
    lo = 1.0 / torch.sqrt(var + dvar + eps)
    hi = 1.0 / torch.sqrt((var - dvar).clamp_min(0) + eps)
    return torch.maximum(hi - ref, ref - lo) + 2 * U32 * hi


def uncentred_bound(d):
    """dvar of var = <T_k, wq_k> / M - mean^2 with T an fp32 chain (the generic path before it was centred)"""
    wq = d['w'].to(BF).double().abs()
    return (d['p'] + 2) * U32 * ((wq @ d['Z'].double().abs()) * wq).sum(1) / d['count']


def gram_finalize_ref(d, momentum=MOMENTUM, eps=EPS, running=True, uncentred=None):
    """every output of tok_bn_gram_finalize as an Out; `uncentred` (default: the path that serves p): the variance bound of the
    uncentred form"""
    p, m = d['p'], float(d['count'])
    Z, zs, wq = d['Z'].double(), d['zsum'].double(), d['w'].to(BF).double()
    gamma, beta = d['gamma'].double(), d['beta'].double()
    epsd, mom = f32(eps), f32(momentum)
    mu = zs / m
    mean = wq @ mu
    var = ((wq @ (Z / m - torch.outer(mu, mu))) * wq).sum(1).clamp_min(0)
    aw = wq.abs()
    magc = ((aw @ (Z.abs() + torch.outer(zs.abs(), zs.abs()) / m)) * aw).sum(1) / m
    dvar = 4 * (p + 4) * U64 * magc
    if (not is_block(p)) if uncentred is None else uncentred:
        dvar = dvar + uncentred_bound(d)
    b_mean = U32 * mean.abs() + (p + 4) * U64 * (aw @ zs.abs()) / m
    rstd = 1.0 / torch.sqrt(var + epsd)
    b_rstd = _rstd_bound(var, dvar, epsd)
    scale = gamma * rstd
    b_scale = gamma.abs() * b_rstd + U32 * scale.abs()
    shift = beta - mean * scale
    cross = mean.abs() * b_scale + (scale.abs() + b_scale) * b_mean
    out = dict(mean=Out(mean, b_mean), rstd=Out(rstd, b_rstd), scale=Out(scale, b_scale),
               shift=Out(shift, cross + U32 * (shift.abs() + cross)), var=Out(var, dvar),
               wz=Out(wq @ Z, (p + 1) * U32 * (aw @ Z.abs())))
    if running:
        unb = m / (m - 1) if m > 1 else 1.0
        one = f32(np.float32(1.0) - np.float32(mom))
        for name, r, s, bs in (('rm', d['rm'].double(), mean, b_mean), ('rv', d['rv'].double(), var * unb, unb * (dvar + U32 * var))):
            ref = one * r + mom * s
            out[name] = Out(ref, 4 * U32 * ((one * r).abs() + (mom * s).abs()) + mom * bs)
    return out


KERNEL_ORDER_MARGIN = 4.0


def large_mean_rstd(d):
    """Out of rstd on the large-mean input.  Block path: the derived bound.  Generic path: no bound small against the value can be
    derived (the worst case of T's fp32 chain is 0.24 of var at P = 72 and above var at P = 320, and a running-error bound over the
    partial sums still 0.2 at P = 320, because the P errors of a row enter <T_k, wq_k> with random signs), so the reference is
    measured against itself: the same formula in the kernel's operation order on the CPU (gram_kernel_order: T by one sequential fp32
    fma chain over q, exactly the order of gemm_f32_kernel, fp64 after it).  The bound of every element is the LARGEST relative
    deviation of that run over the channels, times KERNEL_ORDER_MARGIN = 4: the maximum over the 16 channels measured is a sample of a
    random quantity (the maximum of n such errors grows like sqrt(2 ln n): a factor 2 covers any channel count the unit has), and
    the emulated fma rounds twice where the hardware rounds once (another fp32 ulp of T per step at worst: a factor 2)."""
    r = gram_finalize_ref(d)['rstd']
    if is_block(d['p']):
        return r
    rs = gram_kernel_order(d)[2].double()
    rel = float(((rs - r.ref).abs() / r.ref).max())
    return Out(r.ref, KERNEL_ORDER_MARGIN * rel * r.ref + 2 * U32 * r.ref)


def gram_kernel_order(d, eps=EPS, centred=False):
    """the generic path in the kernels' precision on the CPU: T by an fp32 fma chain over q, then var = <T_k, wq_k> / M - mean^2 in
    fp64 (centred: the fp64 centred row beside it) -> (T, var, rstd as fp32)"""
    p, m = d['p'], float(d['count'])
    Z, zs = d['Z'].numpy(), d['zsum'].numpy().astype(np.float64)
    wq = d['w'].to(BF).float().numpy()
    T = np.zeros((d['k'], p), dtype=np.float32)
    for q in range(p):
        T = (T.astype(np.float64) + wq[:, q:q + 1].astype(np.float64) * Z[q][None, :].astype(np.float64)).astype(np.float32)
    wd = wq.astype(np.float64)
    mean = wd @ zs / m
    if centred:
        var = ((wd @ (Z.astype(np.float64) - np.outer(zs, zs / m))) * wd).sum(1) / m
    else:
        var = (T.astype(np.float64) * wd).sum(1) / m - mean * mean
    var = np.maximum(var, 0)
    rstd = (1.0 / np.sqrt(var + f32(eps))).astype(np.float32)
    return torch.from_numpy(T), torch.from_numpy(var), torch.from_numpy(rstd)


# ---- tok_bn3_bwd_prepare ------------------------------------------------------------------------------------------------------------
def make_prepare(p, k, rows=3, count=4000, seed=0, null_rows=False):
    """operands of tok_bn3_bwd_prepare of `count` rows, built from the fp64 moments of a base sample: G, w, wz, zsum, DISTINCT partial
    rows (row r carries weight (r + 1) / sum, so a skipped or doubled row moves dbeta), mean / rstd of the forward, priors"""
    g = gen(7000 * p + k + 13 * rows + seed)
    nb = min(count, 64)
    s = count / nb
    zb = (torch.randn(nb, p, generator=g, dtype=F64) + 0.2).to(BF).double()
    dzb = torch.randn(nb, k, generator=g, dtype=F64).to(BF).double()
    w = (torch.randn(k, p, generator=g, dtype=F64) * p ** -0.5).float()
    wq = w.to(BF).double()
    Z = (s * (zb.t() @ zb)).float()
    zsum = (s * zb.sum(0)).float()
    G = (s * (dzb.t() @ zb)).float()
    wz = (wq @ Z.double()).float()
    a1 = s * dzb.sum(0)
    wt = torch.arange(1, rows + 1, dtype=F64)
    wt = wt / wt.sum()
    partial = torch.zeros(2, rows, k)
    partial[0] = (wt[:, None] * a1[None, :]).float()
    partial[1] = float('nan')                       # the second half belongs to the other BatchNorm-backward sum: never read here
    y = zb @ wq.t()
    mean = y.mean(0).float()
    rstd = (1.0 / torch.sqrt(y.var(0, unbiased=False) + EPS)).float()
    gamma = (torch.randn(k, generator=g, dtype=F64) * 0.3 + 1).float()
    gamma[0], gamma[min(2, k - 1)] = 0.0, -0.75
    pri = {n: torch.randn(sh, generator=g, dtype=F64).float() for n, sh in (('dgamma', (k,)), ('dbeta', (k,)), ('dw', (k, p)))}
    return dict(p=p, k=k, rows=rows, count=count, G=G, w=w, wz=wz, zsum=zsum, partial=partial, mean=mean, rstd=rstd, gamma=gamma,
                prior=pri)


def bn3_prepare_ref(d, param_acc=0, dw_acc=0):
    """every output of tok_bn3_bwd_prepare as an Out (fp64, the bf16 roundings only in the bounds), following the header of
    csrc/unit3.hip"""
    p, k, rows, m = d['p'], d['k'], d['rows'], float(d['count'])
    G, T, zs = d['G'].double(), d['wz'].double(), d['zsum'].double()
    wq, aw = d['w'].to(BF).double(), d['w'].to(BF).double().abs()
    part = d['partial'][0, :rows].double()
    gamma, mean, rstd = d['gamma'].double(), d['mean'].double(), d['rstd'].double()
    a1, a2 = part.sum(0), (G * wq).sum(1)
    sx = rstd * (a2 - mean * a1)
    pabs = part.abs().sum(0)
    b_a1 = (rows + 2) * U64 * pabs
    b_sx = (p + rows + 6) * U64 * rstd * ((G * wq).abs().sum(1) + mean.abs() * pabs)
    m1, m2 = a1 / m, sx / m
    c1 = gamma * rstd
    c2 = -c1 * rstd * m2
    c3 = -c1 * m1 - c2 * mean
    b_c1 = U32 * c1.abs()
    b_c2 = 4 * U32 * c2.abs() + (c1 * rstd).abs() * b_sx / m
    b_c3 = 4 * U32 * (c1 * m1).abs() + 6 * U32 * (c2 * mean).abs() + c1.abs() * b_a1 / m + mean.abs() * b_c2
    out = {}
    for name, v, b, acc in (('dgamma', sx, U32 * sx.abs() + b_sx, param_acc), ('dbeta', a1, U32 * a1.abs() + b_a1, param_acc)):
        if acc:
            pr = d['prior'][name].double()
            v, b = v + pr, b + U32 * (v + pr).abs()
        out[name] = Out(v, b)
    out['coef'] = Out(torch.stack([c1, c2, c3]), torch.stack([b_c1, b_c2, b_c3]))
    t1, t2, t3 = c1[:, None] * G, c2[:, None] * T, torch.outer(c3, zs)
    dw = t1 + t2 + t3
    b_dw = G.abs() * b_c1[:, None] + T.abs() * b_c2[:, None] + torch.outer(b_c3, zs.abs()) + 3 * U32 * (t1.abs() + t2.abs() + t3.abs())
    if dw_acc:
        pr = d['prior']['dw'].double()
        b_dw = b_dw + U32 * (pr.abs() + dw.abs())
        dw = dw + pr
    out['dw'] = Out(dw, b_dw)
    wa = (c1[:, None] * wq).t().contiguous()
    out['wa'] = Out(wa, (A_BF + 3 * U32) * wa.abs())
    wb = wq.t() @ (c2[:, None] * wq)
    n = k + k // 64 + 8
    out['wb'] = Out(wb, A_BF * wb.abs() + n * U32 * (aw.t() @ (c2.abs()[:, None] * aw)))
    out['cvec'] = Out(c3 @ wq, (n - 4) * U32 * (c3.abs() @ aw) + b_c3 @ aw)
    return out


def unit_autograd(z, w, gamma, beta, shortcut, gout, eps=EPS):
    """fp64 autograd of relu(batch_norm(z w^T) + shortcut) against gout -> dict(dz = relu mask * gout, d(z), dW, dgamma, dbeta, y stats)"""
    zz, ww, gg, bb = (t.double().clone().requires_grad_() for t in (z, w, gamma, beta))
    y = zz @ ww.t()
    out = torch.relu(torch.nn.functional.batch_norm(y, None, None, gg, bb, True, 0.0, eps) + shortcut.double())
    out.backward(gout.double())
    return dict(dz=(out > 0).double() * gout.double(), dx=zz.grad, dw=ww.grad, dgamma=gg.grad, dbeta=bb.grad,
                mean=y.detach().mean(0), var=y.detach().var(0, unbiased=False))


@functools.lru_cache(maxsize=None)
def make_chain(m, p, k):
    """the unit relu(batch_norm(z wq^T) + shortcut) on m rows and its fp64 backward against a bf16 d(out): inputs of the chain of
    kernels (z, dout, the ReLU mask, w, gamma), fp64 results (dz, Z, G, dx, dw, dgamma, dbeta) and element-wise bounds of the chain's
    final outputs.  Sources of error, in order of size (mag = |dz| |wa|^T + |z| |wb| + |cvec|, t1 = dz wa^T):
      wa, wb rounded to bf16, element by element:        A_BF (|dz| |wa|^T + |z| |wb|)
      tok_conv_dgrad stores bf16(t1), tok_conv_dgrad_bias reads it back and stores bf16 of the sum:   A_BF |t1| + A_BF |dx|
      every fp32 quantity in between (Z, G, zsum, the partial rows, the statistics, the coefficients, the accumulators of the two
      data-gradient products) is a chain of at most m + p + k <= 520 roundings, 3.1e-5 of its magnitude; sx = rstd (a2 - mean a1)
      and var = E[y^2] - mean^2 are differences, whose magnitudes exceed their values by a small factor on this input (|mean| ~ 0.2
      std): CHAIN_F32 = 2^-12 (8 x 3.1e-5) of mag covers them.
    dw, dgamma, dbeta pass through no bf16 rounding: CHAIN_F32 of |c1 G| + |c2 T| + |c3 zsum|, of sum |dz xhat| and of sum |dz|."""
    g = gen(m + 3 * p + k)
    z = (torch.randn(m, p, generator=g, dtype=F64) + 0.2).to(BF)
    w = (torch.randn(k, p, generator=g, dtype=F64) * p ** -0.5).float()
    wq = w.to(BF).double()
    gamma = (torch.randn(k, generator=g, dtype=F64) * 0.3 + 1).float()
    beta = torch.randn(k, generator=g, dtype=F64).float()
    sc = torch.randn(m, k, generator=g, dtype=F64)
    dout = torch.randn(m, k, generator=g, dtype=F64).to(BF)
    a = unit_autograd(z, wq, gamma, beta, sc, dout, eps=f32(EPS))
    zd, dz = z.double(), a['dz']
    mask = dz != 0
    Z, G, zs = zd.t() @ zd, dz.t() @ zd, zd.sum(0)
    rstd = 1.0 / torch.sqrt(a['var'] + f32(EPS))
    ex = dict(p=p, k=k, rows=1, count=m, G=G, w=wq, wz=wq @ Z, zsum=zs, partial=torch.stack([dz.sum(0)[None], dz.sum(0)[None]]),
              mean=a['mean'], rstd=rstd, gamma=gamma, prior={})
    r = bn3_prepare_ref(ex)
    c1, c2, c3 = r['coef'].ref
    wa, wb, cvec = r['wa'].ref, r['wb'].ref, r['cvec'].ref
    t1 = dz @ wa.t()
    rnd = dz.abs() @ wa.abs().t() + zd.abs() @ wb.abs()
    mag = rnd + cvec.abs()
    xhat = (zd @ wq.t() - a['mean']) * rstd
    terms = (c1[:, None] * G).abs() + (c2[:, None] * (wq @ Z)).abs() + torch.outer(c3, zs).abs()
    out = dict(dx=Out(a['dx'], A_BF * (a['dx'].abs() + t1.abs() + rnd) + CHAIN_F32 * mag), dw=Out(a['dw'], CHAIN_F32 * terms),
               dgamma=Out(a['dgamma'], CHAIN_F32 * (dz * xhat).abs().sum(0)), dbeta=Out(a['dbeta'], CHAIN_F32 * dz.abs().sum(0)))
    return dict(m=m, p=p, k=k, z=z, w=w, gamma=gamma, beta=beta, dout=dout, mask=mask, dz=torch.where(mask, dout, torch.zeros_like(dout)), zsum=zs.float(), Z=Z, G=G,
                wa=wa, wb=wb, cvec=cvec, t1=t1, out=out)


CHAIN_F32 = 2.0 ** -12


# ---- gradient clip ------------------------------------------------------------------------------------------------------------------
MAX_PARTIALS = 1024
MIN_PER_BLOCK = 8192
SPAN_LISTS = {
    'one': (1,), 'three': (3,), 'five': (5,),
    'mixed': (1, 2, 3, 4, 5, 7, 8193),
    'tiny300': tuple(int(v) for v in torch.randint(1, 10, (300,), generator=gen(300))),
    'cut_in_group': (8191, 2),
    'cut_at_span': (4097, 4096),
    'zero_block': (8192, 8192, 7),                 # make_spans zeroes the middle span: block 1 sums 0.0 and still writes it
    't8192': (8192,), 't8193': (4096, 4097), 't16384': (5, 16379), 't16385': (16383, 2),
    'cap': (MAX_PARTIALS * MIN_PER_BLOCK,),
    'over_cap': (3, MAX_PARTIALS * MIN_PER_BLOCK - 1, 3),
}


def clip_grid(total):
    return max(1, min(cdiv(total, MIN_PER_BLOCK), MAX_PARTIALS))


def clip_chunk(total):
    return cdiv(total, clip_grid(total))


def make_spans(numels, seed=0):
    """one fp32 vector per span, N(0, 1) scaled per span (0.1 ... 10); the list (8192, 8192, 7) gets an all-zero middle span"""
    g = gen(seed + len(numels))
    vals = [(torch.randn(n, generator=g) * 10.0 ** float(torch.rand((), generator=g) * 2 - 1)) for n in numels]
    if tuple(numels) == SPAN_LISTS['zero_block']:
        vals[1].zero_()
    return vals


def grad_partials_ref(vals, shift=0):
    """(partials fp64 [grid], bounds): the sum of squares of every block's slice of the concatenated spans; `shift` moves every
    slice boundary (the wrong restatement of the CPU tests)"""
    flat = np.concatenate([v.numpy().astype(np.float64) for v in vals])
    total = flat.size
    grid, chunk = clip_grid(total), clip_chunk(total)
    starts = np.cumsum([0] + [v.numel() for v in vals])
    sq = flat * flat
    out, bnd = np.zeros(grid), np.zeros(grid)
    for b in range(grid):
        lo = min(b * chunk + (shift if b else 0), total)
        hi = total if b + 1 == grid else min((b + 1) * chunk + shift, total)
        out[b] = sq[lo:hi].sum()
        met = int(np.searchsorted(starts, hi, 'left') - np.searchsorted(starts, lo, 'right') + 1)
        bnd[b] = (4 * cdiv(hi - lo, 1024) + 6 * met + 10 + 26) * U64 * out[b]
    return torch.from_numpy(out), torch.from_numpy(bnd)


def fold_kernel_order(partials):
    """the fold of tok_grad_clip_coef in its order: thread t adds partials[t], [t + 256], ...; lanes by xor butterfly 32 ... 1;
    waves 0 .. 3 in order"""
    p = np.asarray(partials, dtype=np.float64)
    acc = np.zeros(256)
    for i in range(0, p.size, 256):
        seg = p[i:i + 256]
        acc[:seg.size] = acc[:seg.size] + seg
    v = acc.reshape(4, 64)
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, idx ^ off]
    s = 0.0
    for wv in range(4):
        s = s + v[wv, 0]
    return s


def clip_coef_f32(partials, max_norm):
    """(total_norm, coef) as fp32, formed as include/tok.h states: (float) sqrt(sum), max_norm / (norm + 1e-6f), clamp max 1 (a NaN
    passes the clamp)"""
    with np.errstate(all='ignore'):
        tot = np.float32(np.sqrt(fold_kernel_order(partials)))
        c = np.float32(max_norm) / (tot + np.float32(1e-6))
        c = np.float32(1.0) if c > np.float32(1.0) else np.float32(c)
    return tot, c


def grad_scale_ref(vals, coef):
    """x * coef in fp32 (coef == 1: the same bits)"""
    with np.errstate(all='ignore'):
        return [torch.from_numpy(v.numpy() * np.float32(coef)) for v in vals]


def clamp_ref(x, v):
    """the kernel's clamp in numpy: max with -v, then min with v, NaN kept"""
    x = x.numpy().copy()
    v = np.float32(v)
    x = np.where(x < -v, -v, x)
    return torch.from_numpy(np.where(x > v, v, x).astype(np.float32))


def grad_clamp_ref(vals, v):
    return [torch.clamp_(t.clone(), -float(v), float(v)) for t in vals]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def math_norm(vals):
    return math.sqrt(float(sum((v.double() ** 2).sum() for v in vals)))
