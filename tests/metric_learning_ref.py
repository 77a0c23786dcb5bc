"""fp64 references of the metric-learning entries of csrc/metric.hip (tok_l2norm_*, tok_arcface_margin_*, tok_relevance_matrix*,
tok_contrastive_*, tok_embed_reg_*, tok_ntxent_*, tok_triplet_*) and of the retrieval entries of csrc/retrieval.hip
(tok_sim_matrix, tok_topk_rows, tok_retrieval_nrel, tok_retrieval_eval), the bounds of their contracts, the input makers and plain
fp32 runs of the same formulas (tests/test_metric_learning_ref.py: every reference equals torch's own implementation in fp64,
an fp32 run stays inside HALF of every bound, deliberately wrong variants do not pass).  Plain torch / numpy, no HIP.

Every formula is written ONCE, as a function of the working dtype: in float64 it is the reference, in float32 it is the plain
fp32 run.  Every formula restates the reference project's operation (F.normalize, ArcFaceHead.__add_margin, torch.cdist with the
ContrastiveLoss body, BasePairwiseLoss.regularize, CrossEntropyLoss of the NT-Xent logits, nn.TripletMarginLoss, faiss flat search,
the ranx metrics), not the kernels' loops.  A backward takes the saved tensors the call is given (inv_norm and y, S, lse, dist,
row_reg) and every branch is decided on exactly the numbers the kernel sees (s > 0, the swap choice dpn < dan, `active`, cs > th
and the clamp of 1 - cos^2 compared in fp32), so there is no discontinuity to excuse and NO element is excluded anywhere.

An `Out` is (ref, a, b, wide): |mine - ref| <= a + b (+ wide), all per element and absolute.
  a     A_BF = 2^-8 times the magnitude of every value that is STORED as bf16 on the way (0 for fp32 outputs); an fp32 run has none
  b     U32 = 2^-24 per fp32 operation on the longest path, times the magnitude the operation acts on (the same operation on
        absolute values).  K(c) = cdiv(c, 64) + 6 counts a lane-strided sum of c terms (cdiv(c, 64) fused multiply-adds per lane)
        and the 6-step butterfly; a sequential loop of n adds counts n.  Each rounding of a short element-wise chain is counted
        twice (loss_ref.SHORT): one element can come arbitrarily close to the worst case of so short a chain and the fp32 run must
        stay inside HALF of b.
  wide  ArcFace only, see arcface_fwd_ref.
sqrtf and `/` are correctly rounded in this build: __graft_entry__.build() compiles with `-O3 -std=c++17` and nothing that relaxes
them (no -ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt; hipcc's default is correctly rounded), and the device assembly
build() keeps next to metric.hip.o shows it: 11 v_div_scale_f32 / v_div_fmas_f32 / v_div_fixup_f32 division sequences, 9 v_sqrt_f32
each followed by its two correction fmas and compare-selects, and no v_rsq_f32.
Each counts one rounding.  expf and logf are the measured constants of loss_ref (E_EXP, E_LOG: twice the maxima in
profiles/loss_contract_intrinsics.json); NT-Xent feeds logf a sum in [1, n], n <= 1024 (inside the measured [1, 1024]) and expf
arguments far below -104 (un-normalised embeddings, the -1e9 diagonal): that range was measured for this module
(tools/ubench/loss_intrinsics.hip, "expf_far_tail_over_fltmin": every result within that many 2^-126 of the true value, which is
below 2^-149) and is covered by loss_ref.TAIL = 2 x 2^-126 per exponential.

Derivations (x~ is the fp32 value, all errors to first order; the products of two bf16 values are exact in fp32):
l2norm fwd     ss = sum x^2 >= 0: relative K.  sqrt halves it and rounds once, fmaxf is exact, 1 / . rounds once:
               inv_norm  b = (K / 2 + SHORT 2) |inv|;  y = x inv, one more product: b = (K / 2 + SHORT 3) |y|, a = A_BF |y| for bf16
               rows.  Pad columns of y are written 0.  A zero row gives y = 0 exactly (bound 0) and inv = 1 / eps.
l2norm bwd     dot = <dy, y>: K D, D = sum |dy y|.  (dy - y dot) inv: the product y dot, the difference and the product with inv:
               b = |inv| (K |y| D + SHORT 3 (|dy| + |y| D)).  accumulate: + prior, one more sum: SHORT (|v| + |prior|); a on the total.
               Pad columns: written 0 when fresh, re-stored as read under accumulate (unchanged; include/tok.h).
ArcFace fwd    target column, cs > th (easy: cs > 0): phi = bf16(cs cos_m - sn sin_m), sn = sqrt(clamp(1 - cs^2, 0, 1)).  1 - cs^2 is one
               rounding (cs^2 is exact), sqrt halves and rounds: sn carries 1.5; the two products and the difference: the value
               BEFORE the rounding of phi is within d_pre = SHORT (2 |cs cos_m| + 3 |sn sin_m|) U32 of the fp64 one.  The reference
               rounds its own fp64 value to bf16: the two agree unless a bf16 rounding tie lies within d_pre of the fp64 value, and
               then they differ by one bf16 spacing: `wide` = that spacing times |scale| on those elements only (counted by the tests:
               a handful), 0 everywhere else.  Then v * scale: one product (and cs - mm in the hard fallback): b = SHORT 2 |out|,
               a = A_BF |out|.  Targets outside [0, classes) change no column; pad columns are 0.
ArcFace bwd    d = cos_m + cs / sqrt(q) sin_m where the kernel's fp32 q = 1 - cs^2 lies in (0, 1), cos_m where it does not (cs = +-1, and
               |cs| < 2^-12.5 whose q rounds to 1: the branch is taken on the fp32 q), 1 off the target column and in the fallback.
               q, sqrt, the quotient, two products and the sum, then dout * scale * d:
               b = SHORT |dout scale| (3 |cos_m| + 6 |cs / sqrt(q) sin_m|) on the phi branch, SHORT 2 |g| elsewhere; a = A_BF |g|.
contrastive    t = e1_ik - e2_jk is one rounding (twice in t^2), ss = sum t^2 >= 0: relative K + 2; S = sqrt(ss): b = ((K + 2) / 2 + 1) S.
               term_j = (1 - r) relu(mu - S)^2 + r ss: h = relu(mu - S) carries err(S) + |mu - S| (continuous at the margin), h^2 twice
               that relative plus a product, two more products and a sum; the row adds n2 terms in sequence:
               row_loss  b = sum_j [(1 - r) (2 h (err S + |mu - S|) + 4 h^2) + r ss (K + 6)] + n2 row_loss.
               backward, on the S and R it is given: dls = -2 (1 - r) relu(mu - S) + 2 r S (a difference, four products, a sum),
               w = dls / S where S > 0 else 0; acc = sum_o w (me - other) in sequence (`nother` fused multiply-adds, each difference
               one rounding), g = gscale / n1 and the product: b = |g| (nother + 10) sum_o |dls|/S |me - other|, a = A_BF |ref|.
               same tensor: de1 is stored as bf16 between the two launches and the second adds onto it:
               a = A_BF (|first part| + |total|), b += SHORT (|first| + |second|).
embed reg      L1: sum |e|: K row_reg.  L2: sqrt(sum e^2): the squares may or may not be fused: (K + 1) / 2 + 1.
               backward L1: sign(e) (gscale coeff): one product; L2: g e / reg_i: three; SHORT each, a = A_BF; zero row and -0.0: 0.
NT-Xent fwd    s_ij = <e_i, e_j> (1 / T): K + 2 on M_ij = sum_k |e_ik e_jk| / T =: es_ij (1 / T is one rounding, the product another).
               lse = max + log(sum_j exp(s_ij - max)) by the online rule den <- den exp(mx - nm) + exp(s - nm):
                 * through the logits: sum_j p_ij es_ij (d lse / d s_j = p_j)
                 * every term: E_EXP and the rounding of its argument |s_j - max|, weighted p_j; below 2^-126: TAIL each (n TAIL)
                 * every rescale (the running maximum rises `rises` times, counted on the fp64 logits, + 1 for a tie seen the other
                   way): E_EXP, its argument (together at most the span max - first logit) and the product: rises (E_EXP + 1) + span
                 * n adds in sequence: n;  log: E_LOG max(1, log den), den in [1, n];  max + log den: |lse|
               row_loss = lse - s_i,label: + es_i,label + |row_loss|.
NT-Xent bwd    of the lse it is given: w_ij = (exp(s_ij - lse_i) - [j = label i]) + (exp(s_ij - lse_j) - [i = label j]): each exponential
               E_EXP + |s - lse| (the rounding of the argument) + es_ij relative, TAIL absolute, three sums;
               acc_k = sum_j w_ij e_jk in sequence: n;  g = gscale (1 / T) / n and the product: 4:
               b = |g| sum_j (err w_ij + (n + 4) |w|_ij) |e_jk|, |w| = p + [..] + p' + [..];  a = A_BF |ref|; pad columns 0.
triplet fwd    x = a - p + eps: two roundings, absolute ex = (|a - p| + |x|); ss = sum x^2: sum 2 |x| ex + K ss; dist = sqrt(ss):
               err dist = (sum 2 |x| ex + K ss) / (2 dist) + dist (0 where dist = 0: anchor == positive with eps = 0 is exact).
               row_loss = relu(d_ap - d_neg + margin), d_neg = min(d_an, d_pn) under swap (continuous): err d_ap + err d_an + err d_pn
               (the two candidates of the min) + SHORT (|d_ap - d_neg| + |row_loss|).
triplet bwd    on the dist it is given; swap and `active` decided on those fp32 numbers, (d_ap - d_neg) + margin > 0 evaluated in
               fp32.  up = x / d: ex / d + |up|; two differences; g = gscale / rows and the product:
               b = SHORT |g| (sum over the two directions of (ex / d + 4 |u|)), a = A_BF |ref|; inactive rows and pad columns exactly 0.
loss[0]        of every loss, and out[0] of the regulariser: against the fp64 mean of the kernel's OWN row values; the fold is
               fp64, so one fp32 rounding (U32 |mean|, and 2^-40 for the fold).
sim matrix     inner product: d fused multiply-adds in sequence: b = d sum |q g|.  L2: t = q - g one rounding (twice in t^2) and
               d steps: b = (d + 2) sum t^2.  fp32 outputs, pad columns untouched.
top-k, n_rel   exact.  eval: the arithmetic is fp64 on the device (log2 of 2 .. k + 1 within a few 2^-53, k + 2 operations): 2^-40
               covers it; the cast of the result to fp32 is U32 |v|."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from helpers import A_BF, BF, F32, U32, cdiv
from loss_ref import E_EXP, E_LOG, SHORT, TAIL, bounded, flush_record  # noqa: F401  (flush_record: used by the GPU module)

F64 = torch.float64
I64 = torch.int64


def K(c):
    """roundings of a lane-strided sum of c terms: cdiv(c, 64) per lane and the 6-step butterfly"""
    return cdiv(c, 64) + 6


def f32v(v):
    """the value a float argument of the C ABI has once it is passed"""
    return float(np.float32(v))


def bf(t):
    return t.to(BF)


class Out:
    def __init__(self, ref, a=None, b=None, wide=None):
        self.ref = ref.double()
        z = torch.zeros_like(self.ref)
        self.a = z if a is None else a.double().expand_as(self.ref)
        self.b = z if b is None else b.double().expand_as(self.ref)
        self.wide = z if wide is None else wide.double().expand_as(self.ref)

    def bound(self, frac=1.0, rounded=True):
        return (self.a if rounded else 0.0) + frac * self.b + self.wide


def check(tag, what, mine, out, frac=1.0, rounded=True):
    """|mine - ref| <= bound on EVERY element (helpers.assert_bounded through loss_ref.bounded: the worst ratio of (tag, what) is
    kept for the parity record).  frac = 0.5, rounded = False: what an fp32 run has to meet."""
    return bounded(mine, out.ref, out.bound(frac, rounded), 0.0, 1.0, what, tag)


def check_mean(tag, what, value, own_rows):
    """loss[0] against the fp64 mean of the kernel's own row values"""
    mean = own_rows.double().cpu().mean().reshape(1)
    return bounded(value.double().cpu().reshape(1), mean, mean.abs(), U32, 2.0 ** -40, what, tag)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- l2norm ----------------------------------------------------------------------------------------------------------------------
def make_l2norm(rows, c, f32, seed, eps=1e-12):
    """rows of norm ~ sqrt(c); planted: row 0 all zero (rows > 1), row 2 tiny (norm < 1: the clamp branch when eps = 1)"""
    g = gen(seed)
    x = torch.randn(rows, c, generator=g)
    if rows > 1:
        x[0] = 0
    if rows > 2:
        x[2] = x[2] * (0.25 / max(float(x[2].norm()), 1e-6))
    x = x if f32 else bf(x)
    dy = torch.randn(rows, c, generator=g)
    prior = torch.randn(rows, c, generator=g)
    return x, (dy if f32 else bf(dy)), (prior if f32 else bf(prior))


def l2norm_fwd(x, eps, dt=F64):
    """F.normalize(x, dim=1, eps): (1 / max(||x||, eps), x / max(||x||, eps))"""
    xd = x.to(dt)
    inv = 1.0 / xd.pow(2).sum(1).sqrt().clamp_min(f32v(eps))
    return inv, xd * inv[:, None]


def l2norm_fwd_ref(x, eps):
    inv, y = l2norm_fwd(x, eps)
    k = K(x.shape[1])
    return dict(inv_norm=Out(inv, b=(k / 2 + SHORT * 2) * U32 * inv.abs()),
                y=Out(y, a=A_BF * y.abs() if x.dtype == BF else None, b=(k / 2 + SHORT * 3) * U32 * y.abs()))


def l2norm_bwd(dy, y, inv, prior=None, dt=F64):
    """(dy - y <y, dy>) inv of the saved y and inv_norm (+ prior)"""
    g, yy = dy.to(dt), y.to(dt)
    v = (g - yy * (g * yy).sum(1, keepdim=True)) * inv.to(dt)[:, None]
    return v if prior is None else v + prior.to(dt)


def l2norm_bwd_ref(dy, y, inv, prior=None):
    g, yy, iv = dy.double().abs(), y.double().abs(), inv.double().abs()[:, None]
    v = l2norm_bwd(dy, y, inv)
    D = (g * yy).sum(1, keepdim=True)
    b = U32 * iv * (K(dy.shape[1]) * yy * D + SHORT * 3 * (g + yy * D))
    ref = v
    if prior is not None:
        ref = v + prior.double()
        b = b + SHORT * U32 * (v.abs() + prior.double().abs())
    return dict(dx=Out(ref, a=A_BF * ref.abs() if dy.dtype == BF else None, b=b))


# ---- ArcFace margin ------------------------------------------------------------------------------------------------------------
class ArcP:
    """the float constants as the C ABI receives them (engine/metric.py: cos m, sin m, cos(pi - m), sin(pi - m) m)"""

    def __init__(self, m=0.5, scale=30.0, easy=0, th=None):
        self.cos_m, self.sin_m = f32v(math.cos(m)), f32v(math.sin(m))
        self.th = f32v(math.cos(math.pi - m) if th is None else th)
        self.mm, self.scale, self.easy = f32v(math.sin(math.pi - m) * m), f32v(scale), int(easy)

    def args(self):
        return self.cos_m, self.sin_m, self.th, self.mm, self.easy, self.scale


def bf_neighbours(v):
    """(the bf16 value at or below v, the next one above)"""
    lo = torch.tensor([v], dtype=F32).to(BF)
    if float(lo) > v:
        lo = (lo.view(torch.int16) + (1 if v < 0 else -1)).view(BF)
    hi = (lo.view(torch.int16) + (-1 if float(lo) < 0 else 1)).view(BF)
    return float(lo), float(hi)


def make_arcface(rows, classes, p, seed):
    """cosines in [-1, 1] and targets.  Planted on the target column of the first rows: cos = 1, -1, 0, th rounded to bf16 (== th when th
    is a bf16 value) and its two bf16 neighbours, 2^-14 (its fp32 1 - cos^2 is 1); row 7 has target -1, row 8 target == classes"""
    g = gen(seed)
    cs = bf(torch.rand(rows, classes, generator=g) * 2 - 1)
    t = torch.randint(0, classes, (rows,), generator=g)
    lo, hi = bf_neighbours(p.th)
    thb = float(torch.tensor([p.th]).to(BF))
    below = bf_neighbours(thb - abs(thb) * 2.0 ** -10)[0]
    above = bf_neighbours(thb)[1]
    for r, v in enumerate((1.0, -1.0, 0.0, thb, below, above, 2.0 ** -14)):
        if r < rows:
            cs[r, t[r]] = v
    if rows > 7:
        t[7] = -1
    if rows > 8:
        t[8] = classes
    dout = bf(torch.randn(rows, classes, generator=g))
    return cs, t, dout


def _onehot(t, rows, classes):
    oh = torch.zeros(rows, classes, dtype=torch.bool)
    ok = (t >= 0) & (t < classes)
    oh[torch.arange(rows)[ok], t[ok]] = True
    return oh


def _arc_use(cos, p):
    c32 = cos.float()
    return (c32 > 0) if p.easy else (c32 > torch.tensor(p.th, dtype=F32))


def arcface_fwd(cos, t, p, dt=F64, round_phi=True):
    """__add_margin: phi = cos(theta + m), cast to the dtype of the cosines; easy / hard fallback; one-hot select; scale"""
    cs = cos.to(dt)
    sn = (1.0 - cs * cs).clamp(0, 1).sqrt()
    pre = cs * p.cos_m - sn * p.sin_m
    phi = pre.to(BF).to(dt) if round_phi else pre
    phi = torch.where(_arc_use(cos, p), phi, cs if p.easy else cs - p.mm)
    return torch.where(_onehot(t, *cs.shape), phi, cs) * p.scale, pre


def arcface_fwd_ref(cos, t, p):
    out, pre = arcface_fwd(cos, t, p)
    cs = cos.double()
    sn = (1.0 - cs * cs).clamp(0, 1).sqrt()
    d_pre = SHORT * U32 * (2 * (cs * p.cos_m).abs() + 3 * (sn * p.sin_m).abs())
    phi = pre.to(BF).double()
    _, e = torch.frexp(torch.maximum(pre.abs(), phi.abs()))
    ulp = torch.where((pre != 0) | (phi != 0), torch.ldexp(torch.ones_like(pre), e - 8), torch.zeros_like(pre))
    near_tie = (ulp / 2 - (pre - phi).abs()) <= d_pre
    on_phi = _onehot(t, *cs.shape) & _arc_use(cos, p)
    wide = torch.where(on_phi & near_tie, ulp * abs(p.scale), torch.zeros_like(pre))
    return dict(out=Out(out, a=A_BF * out.abs(), b=SHORT * 2 * U32 * out.abs(), wide=wide)), int((wide > 0).sum())


def _arc_inside(cos):
    """the clamp of 1 - cos^2 as the kernel sees it: its fp32 q in (0, 1)"""
    c32 = cos.float()
    q32 = 1.0 - c32 * c32
    return (q32 > 0) & (q32 < 1)


def arcface_bwd(cos, t, dout, p, dt=F64):
    """d out / d cos: scale (cos_m + cos / sqrt(1 - cos^2) sin_m) on the phi branch, the sine term's derivative 0 where
    1 - cos^2 is outside (0, 1) (the rule documented in csrc/metric.hip: autograd of the clamp is not finite at cos = +-1)"""
    cs = cos.to(dt)
    q = (1.0 - cs * cs)
    inside = _arc_inside(cos)
    dsn = torch.where(inside, cs / torch.where(inside, q, torch.ones_like(q)).sqrt(), torch.zeros_like(cs))
    d = torch.where(_onehot(t, *cs.shape) & _arc_use(cos, p), p.cos_m + dsn * p.sin_m, torch.ones_like(cs))
    return dout.to(dt) * p.scale * d, dsn


def arcface_bwd_ref(cos, t, dout, p):
    g, dsn = arcface_bwd(cos, t, dout, p)
    on_phi = _onehot(t, *g.shape) & _arc_use(cos, p)
    gs = (dout.double() * p.scale).abs()
    b = torch.where(on_phi, SHORT * gs * (3 * abs(p.cos_m) + 6 * (dsn * p.sin_m).abs()), SHORT * 2 * g.abs()) * U32
    return dict(dcos=Out(g, a=A_BF * g.abs(), b=b))


# ---- relevance matrices (exact) ----------------------------------------------------------------------------------------------------
def make_labels(na, nb, seed):
    """int64 labels from a small set whose members differ only above bit 32 (a 32-bit comparison would call them equal)"""
    g = gen(seed)
    pool = torch.tensor([3, 3 + 2 ** 32, 3 + 2 ** 40, 7, -5, 2 ** 33])
    return pool[torch.randint(0, len(pool), (na,), generator=g)], pool[torch.randint(0, len(pool), (nb,), generator=g)]


def relevance(la, lb):
    return (la[:, None] == lb[None, :]).to(F32)


def make_multilabel(na, nb, classes, seed):
    """0/1 and small dyadic label matrices whose dot products are exact in fp32 and fp64 alike; planted: a row of zeros in ya
    and a -0.5 entry in yb (a product sum of exactly 0 or below is NOT relevant)"""
    g = gen(seed)
    vals = torch.tensor([0.0, 0.0, 1.0, 0.5, 0.25])
    ya = vals[torch.randint(0, 5, (na, classes), generator=g)]
    yb = vals[torch.randint(0, 5, (nb, classes), generator=g)]
    ya[0] = 0
    yb[nb - 1, classes - 1] = -0.5
    if na > 1:
        ya[na - 1] = 0
        ya[na - 1, classes - 1] = 1.0         # its only product with the last row of yb is negative
    return ya, yb


def relevance_ml(ya, yb, dt=F64):
    """pairwise_task.py: R = (ya yb^T > 0)"""
    return (ya.to(dt) @ yb.to(dt).t() > 0).to(F32)


# ---- contrastive -------------------------------------------------------------------------------------------------------------------
def make_contrastive(n1, n2, d, seed, same=False, margin=1.0, r_mode='mixed'):
    """embeddings of norm ~ margin so that both sides of the hinge occur.  Planted (where the rows exist): e2[0] == e1[0] with
    R = 0 and e2[1] == e1[1] with R = 1 (S == 0 on both kinds of pair); e1[2] - e2[2] = margin on the first coordinate alone with
    R = 0 (a pair exactly at the margin).  same: e2 is e1 (the diagonal is S == 0)."""
    g = gen(seed)
    s = 0.6 * margin / math.sqrt(d)
    e1 = bf(torch.randn(n1, d, generator=g) * s)
    e2 = e1.clone() if same else bf(torch.randn(n2, d, generator=g) * s)
    R = (torch.rand(n1, n2, generator=g) < 0.4).float()
    if r_mode != 'mixed':
        R[:] = float(r_mode)
    if not same:
        for i, r in ((0, 0.0), (1, 1.0)):
            if i < min(n1, n2):
                e2[i] = e1[i]
                R[i, i] = r if r_mode == 'mixed' else R[i, i]
        if min(n1, n2) > 2:
            e2[2] = e1[2]
            e1[2, 0], e2[2, 0] = 0.25 + margin, 0.25
            R[2, 2] = 0.0 if r_mode == 'mixed' else R[2, 2]
    else:
        R = ((R + R.t()) > 0).float()
        R.fill_diagonal_(1.0 if r_mode != '0' else 0.0)
    return e1, e2, R


def contrastive_fwd(e1, e2, R, mu, dt=F64):
    """S = cdist(e1, e2); row_loss = sum_j (1 - R) relu(mu - S)^2 + R S^2   (ContrastiveLoss, the mean over rows is loss[0])"""
    a, b, r = e1.to(dt), e2.to(dt), R.to(dt)
    ss = (a[:, None, :] - b[None, :, :]).pow(2).sum(-1)
    S = ss.sqrt()
    return S, ((1 - r) * (f32v(mu) - S).clamp_min(0).pow(2) + r * ss).sum(1)


def contrastive_fwd_ref(e1, e2, R, mu):
    S, rl = contrastive_fwd(e1, e2, R, mu)
    k, n2, r = K(e1.shape[1]), e2.shape[0], R.double()
    e_s = ((k + 2) / 2 + 1) * S
    h = (f32v(mu) - S).clamp_min(0)
    m = ((1 - r) * (2 * h * (e_s + (f32v(mu) - S).abs()) + 4 * h * h) + r * S * S * (k + 6)).sum(1) + n2 * rl
    return dict(S=Out(S, b=U32 * e_s), row_loss=Out(rl, b=U32 * m))


def contrastive_bwd(e1, e2, R, S, mu, gs, dt=F64, scale_n1=True):
    """autograd of mean_i row_loss_i through S = cdist, given S: w = dL/dS / S (0 where the given S is 0: cdist's subgradient)"""
    a, b, r, s = e1.to(dt), e2.to(dt), R.to(dt), S.to(dt)
    g = gs / a.shape[0] if scale_n1 else gs
    dls = -2 * (1 - r) * (f32v(mu) - s).clamp_min(0) + 2 * r * s
    pos = S > 0
    w = torch.where(pos, dls / torch.where(pos, s, torch.ones_like(s)), torch.zeros_like(s))
    diff = a[:, None, :] - b[None, :, :]
    return (w[:, :, None] * diff).sum(1) * g, -(w[:, :, None] * diff).sum(0) * g


def contrastive_bwd_ref(e1, e2, R, S, mu, gs, same=False):
    g1, g2 = contrastive_bwd(e1, e2, R, S, mu, gs)
    a, b, r, s = e1.double(), e2.double(), R.double(), S.double()
    n1, n2 = a.shape[0], b.shape[0]
    pos = S > 0
    wm = torch.where(pos, (2 * (1 - r) * (f32v(mu) - s).clamp_min(0) + 2 * r * s) / torch.where(pos, s, torch.ones_like(s)), torch.zeros_like(s))
    ad = (a[:, None, :] - b[None, :, :]).abs() * wm[:, :, None]
    gg = abs(gs) / n1
    b1, b2 = U32 * gg * (n2 + 10) * ad.sum(1), U32 * gg * (n1 + 10) * ad.sum(0)
    if same:
        tot = g1 + g2
        return dict(de1=Out(tot, a=A_BF * (g1.abs() + tot.abs()), b=b1 + b2 + SHORT * U32 * (g1.abs() + g2.abs())))
    return dict(de1=Out(g1, a=A_BF * g1.abs(), b=b1), de2=Out(g2, a=A_BF * g2.abs(), b=b2))


# ---- embedding regulariser -----------------------------------------------------------------------------------------------------
def make_embed(n, d, seed):
    """planted: row 0 zero (n > 1), element [n - 1][0] exactly -0.0"""
    e = bf(torch.randn(n, d, generator=gen(seed)))
    if n > 1:
        e[0] = 0
    e[n - 1, 0] = -0.0
    return e


def embed_reg_fwd(e, mode, dt=F64):
    """BasePairwiseLoss.regularize: 'L1' sum |e| per row, 'L2' ||e||_2 per row"""
    x = e.to(dt)
    return x.abs().sum(1) if mode == 1 else x.pow(2).sum(1).sqrt()


def embed_reg_fwd_ref(e, mode):
    rr, k = embed_reg_fwd(e, mode), K(e.shape[1])
    return dict(row_reg=Out(rr, b=U32 * (k if mode == 1 else (k + 1) / 2 + 1) * rr))


def embed_reg_bwd(e, row_reg, gs, coeff, mode, dt=F64):
    """gscale coeff sign(e) ('L1');  gscale coeff e / reg_i, 0 on a row whose saved reg_i is 0 ('L2')"""
    x, g = e.to(dt), f32v(gs) * f32v(coeff)
    if mode == 1:
        return torch.sign(x) * g
    nr = row_reg.to(dt)[:, None]
    pos = (row_reg > 0)[:, None]
    return torch.where(pos, g * x / torch.where(pos, nr, torch.ones_like(nr)), torch.zeros_like(x))


def embed_reg_bwd_ref(e, row_reg, gs, coeff, mode):
    v = embed_reg_bwd(e, row_reg, gs, coeff, mode)
    return dict(de=Out(v, a=A_BF * v.abs(), b=SHORT * (1 if mode == 1 else 3) * U32 * v.abs()))


# ---- NT-Xent ---------------------------------------------------------------------------------------------------------------------
def make_ntxent(n, d, seed, norm=1.0):
    """cat(emb1, emb2) [n][d] with rows of the given norm, the second half a noisy copy of the first (positives are close);
    planted: rows 0 and 1 identical (n > 2)"""
    g = gen(seed)
    h = n // 2
    a = F.normalize(torch.randn(h, d, generator=g), dim=1)
    b = F.normalize(a + 0.3 * torch.randn(h, d, generator=g) / math.sqrt(d), dim=1)
    e = torch.cat([a, b]) * norm
    if n > 2:
        e[1] = e[0]
    return bf(e)


def ntxent_logits(e, t, dt=F64):
    x = e.to(dt)
    n = x.shape[0]
    z = (x @ x.t()) * (1.0 / f32v(t) if dt == F64 else float(np.float32(1.0) / np.float32(t)))
    z = z.masked_fill(torch.eye(n, dtype=torch.bool), -1e9)
    return z, (torch.arange(n) + n // 2) % n


def ntxent_fwd(e, t, dt=F64):
    """NT_XentLoss: CrossEntropyLoss(logits with the diagonal at -1e9, label(i) = (i + B) mod 2B) per row"""
    z, lab = ntxent_logits(e, t, dt)
    lse = torch.logsumexp(z, 1)
    return lse, lse - z.gather(1, lab[:, None])[:, 0]


def _ntx_es(e, t):
    x = e.double().abs()
    return (K(e.shape[1]) + 2) * U32 * (x @ x.t()) / f32v(t)


def ntxent_fwd_ref(e, t):
    z, lab = ntxent_logits(e, t)
    lse, rl = ntxent_fwd(e, t)
    n = z.shape[0]
    es = _ntx_es(e, t)
    p = torch.exp(z - lse[:, None])
    mx = z.max(1).values
    off = torch.where(p > 0, (z - mx[:, None]).abs(), torch.zeros_like(z))
    run = torch.cummax(z, 1).values
    rises = (run[:, 1:] > run[:, :-1]).sum(1) + 1
    first = torch.where(torch.arange(n) == 0, z[:, 1], z[:, 0])
    span = (mx - first).abs()
    den = torch.exp(lse - mx)
    b_lse = (p * es).sum(1) + U32 * (E_EXP + (p * off).sum(1) + rises * (E_EXP + 1) + span + n + E_LOG * torch.log(den).clamp_min(1.0) + lse.abs()) + n * TAIL
    b_rl = b_lse + es.gather(1, lab[:, None])[:, 0] + U32 * rl.abs()
    return dict(lse=Out(lse, b=b_lse), row_loss=Out(rl, b=b_rl))


def ntxent_bwd(e, lse, t, gs, dt=F64, label_shift=0, use_inv_t=True):
    """autograd of mean CE of the symmetric logits, written with the saved lse: d e_i = sum_{j != i} (w_ij + w_ji) e_j g / (n T),
    w_ij = exp(z_ij - lse_i) - [j == label(i)]"""
    x = e.to(dt)
    n = x.shape[0]
    z, lab = ntxent_logits(e, t, dt)
    lab = (lab + label_shift) % n
    l = lse.to(dt)
    oh = torch.zeros(n, n, dtype=dt)
    oh[torch.arange(n), lab] = 1
    w = (torch.exp(z - l[:, None]) - oh)
    w = (w + w.t()).masked_fill(torch.eye(n, dtype=torch.bool), 0)
    return (w @ x) * (gs * (1.0 / f32v(t) if use_inv_t else 1.0) / n)


def ntxent_bwd_ref(e, lse, t, gs):
    d = ntxent_bwd(e, lse, t, gs)
    x = e.double().abs()
    n = x.shape[0]
    z, lab = ntxent_logits(e, t)
    l = lse.double()
    es = _ntx_es(e, t)
    eye = torch.eye(n, dtype=torch.bool)
    oh = torch.zeros(n, n, dtype=F64)
    oh[torch.arange(n), lab] = 1
    p1, p2 = torch.exp(z - l[:, None]), torch.exp(z - l[None, :])
    a1, a2 = (z - l[:, None]).abs().masked_fill(eye, 0), (z - l[None, :]).abs().masked_fill(eye, 0)
    wabs = (p1 + oh + p2 + oh.t()).masked_fill(eye, 0)
    ew = (U32 * (p1 * (E_EXP + a1) + p2 * (E_EXP + a2) + 3 * wabs) + (p1 + p2) * es + 2 * TAIL).masked_fill(eye, 0)
    gg = abs(gs) / f32v(t) / n
    return dict(demb=Out(d, a=A_BF * d.abs(), b=gg * ((ew + (n + 4) * U32 * wabs) @ x)))


# ---- triplet ---------------------------------------------------------------------------------------------------------------------
def make_triplet(rows, d, seed):
    """planted (where the rows exist): row 0 positive == anchor and the negative close by (an active row); row 1 negative far away (loss 0); row 2 d_pn < d_an (the swap takes
    effect); row 3 d_pn > d_an (it does not).  The random rows have both."""
    g = gen(seed)
    a = torch.randn(rows, d, generator=g)
    p = a + 0.5 * torch.randn(rows, d, generator=g)
    n = a + 0.7 * torch.randn(rows, d, generator=g)
    if rows > 0:
        p[0] = a[0]
        n[0] = a[0]
        n[0, :4] += 0.05                    # d_an ~ 0.1 at every d: inside the margin
    if rows > 1:
        n[1] = a[1] + 40.0
    if rows > 2:
        n[2] = p[2] + 0.05 * (n[2] - a[2])
    if rows > 3:
        n[3] = a[3] + 0.05 * (n[3] - a[3])
        p[3] = a[3] + 3.0 * (p[3] - a[3])
    return bf(a), bf(p), bf(n)


def triplet_fwd(a, p, n, margin, eps, swap, dt=F64):
    """nn.TripletMarginLoss(p=2): pairwise_distance(x, y) = ||x - y + eps||; swap: d_neg = min(d_an, d_pn)"""
    A, Pp, N = a.to(dt), p.to(dt), n.to(dt)
    ep = f32v(eps)
    dist = torch.stack([(A - Pp + ep).norm(dim=1), (A - N + ep).norm(dim=1), (Pp - N + ep).norm(dim=1)], 1)
    dneg = torch.minimum(dist[:, 1], dist[:, 2]) if swap else dist[:, 1]
    return dist, (dist[:, 0] - dneg + f32v(margin)).clamp_min(0)


def _trip_parts(a, p, n, eps):
    A, Pp, N = a.double(), p.double(), n.double()
    ep = f32v(eps)
    out = []
    for u, v in ((A, Pp), (A, N), (Pp, N)):
        x = u - v + ep
        out.append((x, (u - v).abs() + x.abs()))
    return out


def triplet_fwd_ref(a, p, n, margin, eps, swap):
    dist, rl = triplet_fwd(a, p, n, margin, eps, swap)
    k = K(a.shape[1])
    errs = []
    for c, (x, ex) in enumerate(_trip_parts(a, p, n, eps)):
        d_ = dist[:, c]
        num = (2 * x.abs() * ex).sum(1) + k * d_ * d_
        errs.append(torch.where(d_ > 0, num / (2 * torch.where(d_ > 0, d_, torch.ones_like(d_))), torch.zeros_like(d_)) + d_)
    e_d = torch.stack(errs, 1)
    dneg = torch.minimum(dist[:, 1], dist[:, 2]) if swap else dist[:, 1]
    m = e_d[:, 0] + e_d[:, 1] + (e_d[:, 2] if swap else 0) + SHORT * ((dist[:, 0] - dneg).abs() + rl)
    return dict(dist=Out(dist, b=U32 * e_d), row_loss=Out(rl, b=U32 * m))


def triplet_branches(dist, margin, swap):
    """(swap taken, active) on the saved fp32 distances, evaluated in fp32 as the kernel does"""
    d32 = dist.float()
    sw = (d32[:, 2] < d32[:, 1]) if swap else torch.zeros(d32.shape[0], dtype=torch.bool)
    dneg = torch.where(sw, d32[:, 2], d32[:, 1])
    return sw, (d32[:, 0] - dneg + torch.tensor(margin, dtype=F32)) > 0


def triplet_bwd(a, p, n, dist, margin, eps, swap, gs, dt=F64, honour_swap=True, use_eps=True):
    """autograd of mean relu(d_ap - d_neg + margin) given the saved distances: d ||x|| / dx = x / ||x|| (0 where the saved ||x|| is 0)"""
    A, Pp, N, D = a.to(dt), p.to(dt), n.to(dt), dist.to(dt)
    rows = A.shape[0]
    sw, active = triplet_branches(dist, margin, swap)
    if not honour_swap:
        sw = torch.zeros_like(sw)
    ep = f32v(eps) if use_eps else 0.0
    g = torch.where(active, torch.full((rows,), gs / rows, dtype=dt), torch.zeros(rows, dtype=dt))[:, None]

    def unit(x, d_):
        pos = (d_ > 0)[:, None]
        return torch.where(pos, x / torch.where(pos, d_[:, None], torch.ones_like(d_[:, None])), torch.zeros_like(x))
    up = unit(A - Pp + ep, D[:, 0])
    un_a, un_p = unit(A - N + ep, D[:, 1]), unit(Pp - N + ep, D[:, 2])
    s = sw[:, None]
    z = torch.zeros_like(up)
    ga = up - torch.where(s, z, un_a)
    gp = -up - torch.where(s, un_p, z)
    gn = torch.where(s, un_p, un_a)
    return ga * g, gp * g, gn * g


def triplet_bwd_ref(a, p, n, dist, margin, eps, swap, gs):
    ga, gp, gn = triplet_bwd(a, p, n, dist, margin, eps, swap, gs)
    sw, active = triplet_branches(dist, margin, swap)
    D = dist.double()
    parts = _trip_parts(a, p, n, eps)

    def mag(c):
        x, ex = parts[c]
        d_ = D[:, c:c + 1]
        pos = d_ > 0
        return torch.where(pos, (ex + 4 * x.abs()) / torch.where(pos, d_, torch.ones_like(d_)), torch.zeros_like(x))
    s = sw[:, None]
    m_neg = torch.where(s, mag(2), mag(1))
    gg = torch.where(active, abs(gs) / a.shape[0], 0.0)[:, None].double()
    z = torch.zeros_like(m_neg)
    ma, mp, mn = mag(0) + torch.where(s, z, m_neg), mag(0) + torch.where(s, m_neg, z), m_neg
    return dict(d_anchor=Out(ga, a=A_BF * ga.abs(), b=SHORT * U32 * gg * ma),
                d_positive=Out(gp, a=A_BF * gp.abs(), b=SHORT * U32 * gg * mp),
                d_negative=Out(gn, a=A_BF * gn.abs(), b=SHORT * U32 * gg * mn))


# ---- similarity matrix and top-k ---------------------------------------------------------------------------------------------------
def make_sim(nq, ng, d, seed):
    g = gen(seed)
    return torch.randn(nq, d, generator=g), torch.randn(ng, d, generator=g)


def sim_matrix(q, g, metric, dt=F64):
    """faiss IndexFlatIP scores <q, g>; IndexFlatL2 squared distances, negated so that larger is closer"""
    a, b = q.to(dt), g.to(dt)
    return a @ b.t() if metric == 0 else -(a[:, None, :] - b[None, :, :]).pow(2).sum(-1)


def sim_matrix_ref(q, g, metric):
    s, d = sim_matrix(q, g, metric), q.shape[1]
    m = d * (q.double().abs() @ g.double().abs().t()) if metric == 0 else (d + 2) * s.abs()
    return dict(out=Out(s, b=U32 * m))


def make_topk(rows, cols, seed):
    """few distinct values (many ties).  Planted rows: 0 all equal, 1 all -inf, 2 with a +inf, 3 all NaN, 4 of -0.0 and +0.0 only,
    5 with NaN scattered among values"""
    g = gen(seed)
    s = torch.randint(-3, 4, (rows, cols), generator=g).float() * 0.5
    if rows > 0:
        s[0] = 1.5
    if rows > 1:
        s[1] = -math.inf
    if rows > 2:
        s[2, cols // 2] = math.inf
    if rows > 3:
        s[3] = math.nan
    if rows > 4:
        s[4] = 0.0
        s[4, ::2] = -0.0
    if rows > 5:
        s[5, ::3] = math.nan
    return s


def topk_rows(s, k, reverse_ties=False):
    """(vals [rows][k], idx [rows][k]): a stable sort on (value descending, index ascending); NaN never ranks; what is missing is
    (-inf, -1), as faiss pads"""
    sv = s.numpy()
    rows, cols = sv.shape
    vals = np.full((rows, k), -np.inf, np.float32)
    idx = np.full((rows, k), -1, np.int64)
    for r in range(rows):
        live = np.where(~np.isnan(sv[r]))[0]
        if reverse_ties:
            live = live[::-1]
        order = live[np.argsort(-sv[r][live], kind='stable')][:k]
        vals[r, :len(order)], idx[r, :len(order)] = sv[r][order], order
    return torch.from_numpy(vals), torch.from_numpy(idx)


# ---- retrieval: number of relevant vectors and the per-query metrics ---------------------------------------------------------------
KINDS = ('hit_rate', 'precision', 'recall', 'average_precision', 'ndcg')


def nrel(labels, scores, q_row, q_col, keep_self=False):
    """classification data: vectors with the query's label, the query itself excluded; representation data: rows whose score in the
    query's column reaches relevance level 1"""
    if labels is not None:
        same = labels[None, :] == labels[q_row][:, None]
        return (same.sum(1) - (0 if keep_self else 1)).to(torch.int32)
    return (scores[:, q_col] >= 1).sum(0).to(torch.int32)


def retrieval_eval(kind, idx, drop_first, gallery, ng, labels, scores, q_row, q_col, n_rel, ideal, invert_drop=False, ndcg_k_only=False):
    """the header contract in fp64 and integers, one query at a time: the kk - 1 results left after dropping the first (drop_first) or
    the last of the kk found; idx -1 is gallery[ng - 1]; gain = [same label, not the query] or the score where it reaches 1;
    hit_rate, precision (/ k), recall (/ n_rel), average precision (/ n_rel), nDCG = DCG / IDCG over min(k, n_rel) ideal gains."""
    nq, kk = idx.shape
    k = kk - 1
    out = np.zeros(nq, np.float64)
    for qi in range(nq):
        nr = int(n_rel[qi])
        if nr == 0 or k <= 0:
            continue
        first = 1 if bool(drop_first[qi]) != invert_drop else 0
        row = int(q_row[qi])
        hits, ap, dcg = 0, 0.0, 0.0
        for p in range(k):
            li = int(idx[qi, first + p])
            li = ng - 1 if li < 0 else li
            gi = int(gallery[li]) if gallery is not None else li
            if labels is not None:
                gain = 1.0 if (int(labels[gi]) == int(labels[row]) and gi != row) else 0.0
            else:
                gain = float(scores[gi, int(q_col[qi])])
                gain = gain if gain >= 1.0 else 0.0
            if gain > 0:
                hits += 1
                ap += hits / (p + 1)
                dcg += gain / math.log2(p + 2)
        if kind == 0:
            v = 1.0 if hits else 0.0
        elif kind == 1:
            v = hits / k
        elif kind == 2:
            v = hits / nr
        elif kind == 3:
            v = ap / nr
        else:
            ki = k if ndcg_k_only else min(k, nr)
            v = dcg / sum((float(ideal[qi, p]) if ideal is not None else 1.0) / math.log2(p + 2) for p in range(ki))
        out[qi] = v
    return torch.from_numpy(out)


def eval_out(v):
    return Out(v, b=(U32 + 2.0 ** -40) * v.abs())


def make_retrieval(kind_data, n, nq, kk, seed, use_gallery):
    """One evaluation problem.  classification: n labelled vectors (label 9 occurs once: a query with n_rel == 0; label 0 many times:
    n_rel > kk - 1; label 1 twice: n_rel < kk - 1); representation: scores [n][n_cols] with graded gains 1, 2, 3, values just below 1
    (0.99999994: NOT relevant) and an all-zero column.  idx rows hold -1 entries; drop_first is mixed; gallery is NULL or a
    permutation of a subset.  Returns a dict of tensors (idx refers to gallery rows)."""
    g = gen(seed)
    ng = n if not use_gallery else max(n - 3, 1)
    gallery = torch.randperm(n, generator=g)[:ng].to(I64) if use_gallery else None
    q_row = torch.randint(0, n, (nq,), generator=g).to(I64)
    idx = torch.randint(0, ng, (nq, kk), generator=g).to(I64)
    idx[torch.rand(nq, kk, generator=g) < 0.1] = -1
    idx[0, 0] = -1
    drop = (torch.rand(nq, generator=g) < 0.5).to(torch.uint8)
    drop[0] = 1
    if nq > 1:
        drop[1] = 0
    out = dict(n=n, ng=ng, gallery=gallery, q_row=q_row, idx=idx, drop_first=drop, labels=None, scores=None, q_col=None, ideal=None)
    if kind_data == 'classification':
        labels = torch.randint(0, 4, (n,), generator=g).to(I64)
        labels[labels == 1] = 0
        if n > 4:
            labels[0], labels[1], labels[2] = 9, 1, 1
            q_row[0] = 0                                              # n_rel == 0
            if nq > 1:
                q_row[1] = 1                                          # n_rel == 1 < kk - 1
        labels = labels + (2 ** 33) * (labels == 3)                 # a label beyond 32 bits
        out['labels'] = labels
    else:
        n_cols = 5
        vals = torch.tensor([0.0, 0.0, 0.0, 0.99999994, 1.0, 2.0, 3.0])
        scores = vals[torch.randint(0, len(vals), (n, n_cols), generator=g)]
        scores[:, 4] = 0                                              # a query column without relevant rows
        scores[:, 2] = torch.where(scores[:, 2] >= 1, torch.full((), 0.99999994), scores[:, 2])
        scores[n // 2, 2], scores[n - 1, 2] = 2.0, 1.0                # ... and one with two (fewer than kk - 1)
        scores[: max(n - 2, 1), 3] = torch.where(scores[: max(n - 2, 1), 3] >= 1, scores[: max(n - 2, 1), 3], torch.ones(()))  # many relevant
        q_col = torch.randint(0, n_cols, (nq,), generator=g).to(I64)
        q_col[0] = 4
        if nq > 1:
            q_col[1] = 3
        if nq > 2:
            q_col[2] = 2
        out['scores'], out['q_col'] = scores, q_col
        gains = torch.where(scores >= 1, scores, torch.zeros(()))[:, q_col].t().contiguous()       # [nq][n]
        out['ideal'] = torch.sort(gains, 1, descending=True).values[:, :kk - 1].contiguous() if n >= kk - 1 else \
            torch.cat([torch.sort(gains, 1, descending=True).values, torch.zeros(nq, kk - 1 - n)], 1)
    out['n_rel'] = nrel(out['labels'], out['scores'], q_row, out['q_col'])
    return out


# ---- the zero vector under normalize_vectors=True -----------------------------------------------------------------------------------
def zero_vector_problem():
    """a classification set whose row 3 is the zero vector.  The reference's `vectors /= norm` makes that row 0 / 0 = NaN
    (index_base_metric.py:192-193; per row, see the note at the top of oracle/retrieval_ref.py) and every inner product with it NaN.
    What that must score is the oracle's answer: oracle.retrieval_ref.meter_compute(normalize_vectors=True), whose flat_search
    states faiss's rule for a NaN score (never a result; a query without results gets labels -1).  Returns (vectors, labels, k)."""
    rng = np.random.RandomState(3)
    n, d, k = 12, 6, 3
    vec = rng.randn(n, d).astype(np.float32)
    vec[3] = 0
    labels = np.array([0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 0, 0])
    return vec, labels, k


def run_zero_vector_meter(device):
    """{metric: (the meter's value, the oracle's value, the oracle's value for the zero-vector query alone)}"""
    import oracle.retrieval_ref as O
    import torchok_amd.retrieval as RT
    vec, labels, k = zero_vector_problem()
    out = {}
    for name, cls in (('hit_rate', RT.HitAtKMeter), ('precision', RT.PrecisionAtKMeter), ('recall', RT.RecallAtKMeter),
                      ('average_precision', RT.MeanAveragePrecisionAtKMeter), ('ndcg', RT.NDCGAtKMeter)):
        m = cls(dataset_type='classification', k=k, normalize_vectors=True)
        m.update(torch.from_numpy(vec).to(device), group_labels=torch.from_numpy(labels).to(device))
        want, per_q = O.meter_compute(name, vec, 'classification', k=k, group_labels=labels, normalize_vectors=True, per_query=True)
        out[name] = (m.compute(), want, per_q[3])
    return out


# ---- the cases of tests/test_metric_learning_contract_gpu.py (tests/test_metric_learning_ref.py runs the fp32 formulas on the same inputs) ----
ROWS = (1, 5, 8, 131)                       # a lone wave, a ragged last block, a full block, many blocks (four waves per block)
COLS = ((1, 8), (20, 24), (63, 64), (64, 64), (65, 72), (129, 129), (1000, 1000))      # (c, ld): below, at and above the 64 lanes
L2NORM_F32_EXTRA = (3, 2049, 2056)
ARC_CASES = [(5, 7, 8, 'below one block'), (37, 65, 72, 'blocks'), (129, 8131, 8136, 'second trip')]     # rows, classes, ld
CONTRASTIVE_CASES = [(1, 1, 20, 24, False), (5, 3, 63, 64, False), (8, 8, 65, 72, True), (33, 65, 129, 129, False), (300, 7, 20, 24, False)]
NTX_N = (2, 6, 64, 258)
NTX_D = ((20, 24), (64, 64), (961, 968), (1023, 1024), (1024, 1024))
REL_CASES = [(1, 1), (7, 130), (256, 256)]
ML_CLASSES = (1, 5, 80)
SIM_CASES = [(1, 1, 1), (63, 65, 15), (64, 64, 16), (65, 129, 17), (130, 70, 200)]
EVAL_NQ = (1, 5, 257)
GRID_CAP = 4096


def grid_for(total):
    """csrc/metric.hip grid_for: blocks of 256 elements, at most 4096 of them (the kernels stride over the rest)"""
    return min(max(cdiv(total, 256), 1), GRID_CAP)
