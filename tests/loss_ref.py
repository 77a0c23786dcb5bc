"""fp64 references of the loss entries of csrc/loss_*.hip and the metric-count entries of csrc/metric.hip (include/tok.h) on the same bf16-rounded inputs, the
bounds of their contracts, the input makers, and plain fp32 runs of the same formulas (tests/test_loss_ref.py: an fp32 run
stays inside half of every bound, deliberately wrong variants do not pass).  Everything is plain torch and runs on the device of
its inputs (the GPU module keeps the large cases on the device in float64).

Every bound has the form of helpers.assert_bounded, |mine - ref| <= a |ref| + b mag: a = A_BF = 2^-8 for ONE bf16 rounding of a
stored result (0 for fp32 outputs), b = U32 = 2^-24 per fp32 operation on the longest path, and `mag` the per-element count of
those operations times the magnitude they act on, derived next to each use.  One exception, SHORT = 2: an element-wise result
reached through a handful of roundings with no long sum behind it (d(logits) of softmax CE, dx of the regression losses, the add
onto a previous gradient) has each of those roundings counted twice, because one element can come arbitrarily close to the worst
case of so short a chain (a single rounding reaches U32 |x| whenever |x| lies just above a power of two) and
tests/test_loss_ref.py asks that an fp32 run stay inside HALF of every bound.  Sums, folds and the device-function constants are
counted once.  The constants that cannot be derived from the code are the
accuracies of the device math functions (below); an exponential whose true value lies below the smallest normal fp32 number
may come back as anything from 0 to that number (flush to zero), which is the absolute term TAIL.

softmax cross entropy (wave kernel: lane-strided sums and a 64-lane butterfly; thread-per-row kernel: ld sequential adds)
  lse       s = sum_c exp(z_c - max) lies in [1, classes]: every term carries E_EXP and, through the rounding of z_c - max,
            |z_c - max| (both relative, so weighted by the term's share p_c of the sum), the sum `adds` roundings, the logarithm
            E_LOG max(1, log s), max + log s one rounding of |lse|
  row_loss  (1 - s)(lse - z_t) + s (lse - mean z): the error of lse, `adds` roundings in the sum of z and six more
            operations, on the magnitude (1 - s)|lse - z_t| + s (|lse| + mean|z|); exactly 0 on dropped rows
  loss[0]   against the fp64 mean of the kernel's OWN row_loss over the valid rows: the fold is fp64, so one fp32 rounding
  loss[1]   the number of valid rows, exactly
  dlogits   (p - (1 - s) onehot - s / classes) g / n_valid with p = exp(z - lse) of the lse the call is GIVEN: p carries
            E_EXP + SHORT |z - lse|, then two subtractions, 1 - s, s / classes, g / n_valid and the product: SHORT x six roundings of
            (p + (1 - s) onehot + s / classes) |g| / n_valid; one bf16 rounding; pad columns and dropped rows exactly 0

upsample cross entropy: see UpRef; Dice: DiceRef; BCE: bce_ref; regression: reg_ref; counts: counts_ref (exact)."""
import math

import numpy as np
import torch

from helpers import A_BF, BF, U32, assert_bounded, cdiv, record_distance

F64 = torch.float64
SHORT = 2.0                 # see the module docstring
FLT_MIN = 2.0 ** -126

# ---- accuracy of the device math functions, in units of 2^-24 ----------------------------------------------------------------------
# The ROCm device-library documentation installed with the toolchain states no error bounds, so each function was measured once on
# an MI355X against fp64 (tools/ubench/loss_intrinsics.hip, 2^22 points over the range the kernels feed it; the measured maxima are
# kept in profiles/loss_contract_intrinsics.json) and is given a 2x margin here.
#   expf, __expf   relative error of exp(x), x = v - max in [-104, 0], where the result is a normal number; expf also on [0, 88],
#                  the arguments of the sigmoids 1 / (1 + expf(-z)) of Dice and BCE (M_EXP is the larger of the two ranges)
#   logf, __logf   |error| / max(1, |log s|), s in [1, 1024]
#   log1pf         relative error of log1p(u), u = exp(-|x|) in (0, 1]
M_EXP, M_FEXP, M_LOG, M_FLOG, M_L1P = 1.40, 64.5, 3.04, 3.04, 1.05      # measured maxima (rounded up)
E_EXP, E_FEXP, E_LOG, E_FLOG, E_L1P = 2 * M_EXP, 2 * M_FEXP, 2 * M_LOG, 2 * M_FLOG, 2 * M_L1P
TAIL = 2 * FLT_MIN          # |error| of an exponential whose value is below FLT_MIN (measured: __expf flushes it to 0, 1 FLT_MIN)


def bf(t):
    return t.to(BF)


_WORST = {}


def bounded(mine, ref, mag, a, b, what, tag=None):
    """helpers.assert_bounded; with a tag (a kernel family), the worst |err| / bound of (tag, what) over every case that uses the tag is
    kept for flush_record(), which writes one line per family and tensor to the parity record"""
    w = assert_bounded(mine, ref, mag, a, b, what)
    if tag is not None:
        _WORST[(tag, what)] = max(w, _WORST.get((tag, what), 0.0))
    return w


def flush_record():
    for (tag, what), w in _WORST.items():
        record_distance(tag, what, err_over_bound=w)
    _WORST.clear()


def ce_adds(classes, ld=None):
    """longest chain of additions in a sum over the classes: the thread-per-row kernels add ld <= 64 terms in sequence, the wave
    kernel cdiv(classes, 64) per lane and six butterfly steps"""
    return max(min(ld or classes, 64), cdiv(classes, 64) + 6)


# ---- softmax cross entropy ------------------------------------------------------------------------------------------------------
def make_ce(rows, classes, ignore_index, seed):
    """bf16 logits [rows][classes] and int64 targets.  A fifth of the rows ignored; planted (where the row exists): row 0
    ignored, rows 1-3 the labels `classes`, -1 and 2^40 (dropped), row 4 a single +80 among -80s, row 5 constant with the last
    class as target, row 6 -inf on a non-target class, and the last row valid"""
    g = torch.Generator().manual_seed(seed)
    z = bf(torch.randn(rows, classes, generator=g) * 3)
    t = torch.randint(0, classes, (rows,), generator=g)
    t[torch.rand(rows, generator=g) < 0.2] = ignore_index
    for r, lab in ((0, ignore_index), (1, classes), (2, -1), (3, 2 ** 40)):
        if r < rows:
            t[r] = lab
    if rows > 4:
        z[4] = -80.0
        z[4, 4 % classes] = 80.0
        t[4] = seed % classes
    if rows > 5:
        z[5] = 1.5
        t[5] = classes - 1
    if rows > 6 and classes > 1:
        z[6, classes - 1] = -math.inf
        t[6] = 0
    if rows > 7:
        t[rows - 1] = classes - 1
    return z, t


def ce_valid(t, ignore_index, classes):
    return (t != ignore_index) & (t >= 0) & (t < classes)


class CERef:
    """z: bf16 (or already float64) logits [rows][classes].  `slack` (upsample CE): per-element width of the set of legitimate
    values of z, see UpRef."""

    def __init__(self, z, t, ignore_index, s=0.0, e_exp=E_EXP, e_log=E_LOG, adds=None, slack=None):
        zd = z.double()
        rows, classes = zd.shape
        self.s, self.classes, self.e_exp = float(s), classes, e_exp
        self.adds = adds = ce_adds(classes) if adds is None else adds
        mx = zd.max(1, keepdim=True).values
        x = zd - mx
        e = torch.exp(x)
        S = e.sum(1, keepdim=True)
        p = e / S
        self.zd, self.t = zd, t
        self.lse = (mx + torch.log(S))[:, 0]
        self.lse32 = self.lse.float()
        xw = (torch.where(e > 0, x.abs(), torch.zeros_like(x)) * p).sum(1)
        self.b_lse = U32 * (e_exp + xw + adds + e_log * torch.log(S)[:, 0].clamp_min(1.0) + self.lse.abs()) + classes * TAIL
        self.valid = valid = ce_valid(t, ignore_index, classes)
        self.n_valid = int(valid.sum())
        self.tt = tt = t.clamp(0, classes - 1)
        nll = self.lse - zd.gather(1, tt[:, None])[:, 0]
        rl, m_rl = nll, nll.abs()
        if s:
            rl = (1.0 - s) * nll + s * (self.lse - zd.mean(1))
            m_rl = (1.0 - s) * nll.abs() + s * (self.lse.abs() + zd.abs().mean(1))
        zero = torch.zeros_like(rl)
        self.row_loss = torch.where(valid, rl, zero)
        self.inf_rows = valid & torch.isinf(self.row_loss)            # -inf logit under smoothing: +inf, as torch
        self.b_rl = torch.where(valid & ~self.inf_rows, self.b_lse + (adds + 6) * U32 * torch.nan_to_num(m_rl, posinf=0.0), zero)
        self.n_slack, self.w_lse, self.w_rl = 0, zero, zero      # the widening under slack: not part of the fp32 error
        if slack is not None:
            # a legitimate value of z_c anywhere in an interval of width slack_c: lse moves by at most sum_c p_c slack_c exp(slack_c)
            # (mean value theorem: d lse / d z_c = p_c, and p_c grows by at most exp(slack_c) inside the interval); z_t moves too
            w = (p * slack * torch.exp(slack)).sum(1)
            self.w_lse, self.w_rl = w, torch.where(valid, w + slack.gather(1, tt[:, None])[:, 0], zero)
            self.n_slack = int((slack > 0).sum())
        self.slack = slack

    def grad(self, gs=1.0):
        """d(logits) of the lse the backward is given (self.lse32), its magnitude (in units of U32) and, under slack, the
        absolute widening per element"""
        zd, s, classes = self.zd, self.s, self.classes
        l = self.lse32.double()[:, None]
        p = torch.exp(zd - l)
        oh = torch.zeros_like(zd)
        oh.scatter_(1, self.tt[:, None], 1.0)
        v = self.valid[:, None].double()
        k = abs(gs) / max(self.n_valid, 1)
        d = (p - (1.0 - s) * oh - s / classes) * (gs / max(self.n_valid, 1)) * v
        relp = torch.where(p > 0, self.e_exp + SHORT * (zd - l).abs(), torch.zeros_like(p))
        mag = (p * (relp + SHORT * 6.0) + SHORT * 6.0 * ((1.0 - s) * oh + s / classes) + TAIL / U32) * k * v
        wide = None
        if self.slack is not None:
            wide = p * self.slack * torch.exp(self.slack) * k * v
        return d, mag, wide


def check_ce_fwd(tag, ref, lse, row_loss, frac=1.0):
    rec = tag if frac == 1.0 else None
    bounded(lse, ref.lse, frac * ref.b_lse + ref.w_lse, 0.0, 1.0, 'lse', rec)
    rl, fin = row_loss.double().to(ref.lse.device), ~ref.inf_rows
    assert bool((rl[ref.inf_rows] == math.inf).all()), 'row_loss: a -inf logit under label smoothing is +inf'
    assert bool((rl[~ref.valid] == 0).all()), 'row_loss: dropped rows are exactly 0'
    bounded(rl[fin], ref.row_loss[fin], (frac * ref.b_rl + ref.w_rl)[fin], 0.0, 1.0, 'row_loss', rec)


def check_ce_mean(tag, ref, loss, own_row_loss):
    """loss[1] exact; loss[0] against the fp64 mean of the kernel's own row losses over the valid rows: one fp32 rounding (and
    2^-40 for the fp64 fold itself)"""
    loss = loss.double().cpu()
    assert float(loss[1]) == ref.n_valid, f'loss[1] = {float(loss[1])}, {ref.n_valid} valid rows'
    own = own_row_loss.double().to(ref.valid.device)
    if ref.n_valid == 0:
        assert math.isnan(float(loss[0])), 'all rows ignored: the mean is 0 / 0, as torch'
        return
    mean = own[ref.valid].sum() / ref.n_valid
    if bool(ref.inf_rows.any()):
        assert float(loss[0]) == math.inf and float(mean) == math.inf
        return
    bounded(loss[0:1], mean.reshape(1), mean.abs().reshape(1), U32, 2.0 ** -40, 'loss[0] vs its own rows', tag)


def check_ce_bwd(tag, ref, gs, d, frac=1.0, what='dlogits'):
    rec = tag if frac == 1.0 else None
    want, mag, _ = ref.grad(gs)
    d = d.double().to(want.device)
    assert bool((d[~ref.valid] == 0).all()), f'{what}: dropped rows are exactly 0'
    a = A_BF if frac == 1.0 else 0.0
    bounded(d, want, mag, a, frac * U32, what, rec)
    # rows sum to ~0: the sum of the per-element bounds
    lim = (a * want.abs() + frac * U32 * mag).sum(1) + want.sum(1).abs()
    assert bool((d.sum(1).abs() <= lim).all()), f'{what}: a row does not sum to 0 within its bound'


def ce_fp32(z, t, ignore_index, s, wrong=None):
    """the same formulas in fp32, unrounded.  wrong: 's_over_ld' (smoothing spread over the row pitch), 'mean_all_rows'"""
    zf = z.float()
    rows, classes = zf.shape
    mx = zf.max(1, keepdim=True).values
    l = (mx + torch.log(torch.exp(zf - mx).sum(1, keepdim=True)))[:, 0]
    valid = ce_valid(t, ignore_index, classes)
    tt = t.clamp(0, classes - 1)
    rl = l - zf.gather(1, tt[:, None])[:, 0]
    if s:
        rl = (1.0 - s) * rl + s * (l - zf.sum(1) / classes)
    rl = torch.where(valid, rl, torch.zeros(()))
    nv = float(valid.sum())
    den = float(rows) if wrong == 'mean_all_rows' else nv
    loss = torch.tensor([float(rl.double().sum() / den) if den else math.nan, nv])
    return l, rl, loss, den


def ce_fp32_bwd(z, t, ignore_index, s, lse32, den, gs, wrong=None, ld=None):
    zf = z.float()
    rows, classes = zf.shape
    valid = ce_valid(t, ignore_index, classes)
    oh = torch.zeros_like(zf)
    oh.scatter_(1, t.clamp(0, classes - 1)[:, None], 1.0)
    spread = s / (ld if wrong == 's_over_ld' else classes)
    g = torch.tensor(gs, dtype=torch.float32) / torch.tensor(den, dtype=torch.float32)
    return (torch.exp(zf - lse32[:, None]) - (1.0 - s) * oh - spread) * g * valid[:, None]


# ---- cross entropy on bilinearly upsampled logits ---------------------------------------------------------------------------------
def up_axis(n_src, n_dst):
    """ATen's area_pixel_compute_source_index (align_corners = False) in fp32, operation by operation: i0, i1, lambda0, lambda1
    of every destination index.  Part of the contract."""
    f = np.float32
    scale = f(n_src) / f(n_dst)
    s = scale * (np.arange(n_dst, dtype=f) + f(0.5)) - f(0.5)
    s = np.maximum(s, f(0))
    i0 = np.minimum(s.astype(np.int64), n_src - 1)
    i1 = i0 + (i0 < n_src - 1)
    l1 = (s - i0.astype(f)).astype(f)
    return i0, i1, (f(1) - l1).astype(f), l1


def up_tiled_ok(hs, ws, hd, wd):
    """restatement of the launcher's choice in tok_upsample_ce_bwd: the tiled kernel serves a window of UT + 1 = 9 source pixels
    at the larger destination / source ratio r, plus 4, when it fits UWIN = 40 destination pixels, i.e. r <= 4"""
    f = np.float32
    r = max(f(1) / (f(hs) / f(hd)), f(1) / (f(ws) / f(wd)))
    return int(math.ceil(f(9) * r)) + 4 <= 40


def make_up(n, hs, ws, classes, hd, wd, seed, dyadic=False):
    """bf16 low-resolution logits [n][hs][ws][classes], int64 targets [n][hd][wd]: the first two rows and the last column ignored
    (255), the last image ignored whole when n > 1, one label == classes (dropped)"""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(n, hs, ws, classes, generator=g) * 2
    low = (low * 4).round() / 4 if dyadic else low
    t = torch.randint(0, classes, (n, hd, wd), generator=g)
    t[:, :2] = 255
    t[:, :, -1] = 255
    if n > 1:
        t[n - 1] = 255
    if hd > 3 and wd > 2:
        t[0, 3, 1] = classes
    return bf(low), t


def _w_matrix(i0, i1, h, l, n_src):
    W = torch.zeros(len(i0), n_src, dtype=F64)
    idx = torch.arange(len(i0))
    W[idx, torch.from_numpy(i0)] += torch.from_numpy(h.astype(np.float64))
    W[idx, torch.from_numpy(i1)] += torch.from_numpy(l.astype(np.float64))
    return W


class UpRef:
    """fp64 reference of tok_upsample_ce_fwd / _bwd.  The interpolant hy (hx a + lx b) + ly (hx c + lx d) is evaluated in fp64 from
    the fp32 indices and weights; an fp32 evaluation differs from it by at most
        err_v = 4 U32 Mw + 2 (dy + dx) Mmax
    (four roundings along any path on the weighted magnitude Mw; each weight off by at most d = 2 U32 (n_src + 1), one ulp of the
    source coordinate, should the compiler contract scale * (dst + 0.5) - 0.5 into one fused operation; Mmax = the largest corner).
    The kernel rounds its interpolant to bf16: where [v - err_v, v + err_v] contains a bf16 rounding tie both neighbours are
    legitimate and `slack` = their distance for exactly those elements (0 elsewhere, `n_slack` of them), which widens lse, row_loss
    and d(upsampled logits) of that pixel as CERef states.  With `exact` (dyadic inputs, power-of-two scales) the fp32 evaluation
    is asserted to EQUAL the fp64 one and err_v = 0: no slack at all.

    Backward: dlow = adjoint of the interpolation applied to bf16(d upsampled logits), fp32 accumulation over `terms` <= (2 r + 4)^2
    visits, rounded once.  d(upsampled logits) is rounded to bf16 inside the kernel, so the same tie rule applies to it: `dslack` =
    the distance between the bf16 roundings of the two ends of its own error interval.  Bound of an element of dlow:
        A_BF |ref| + U32 (terms + 2) sum w |d| + (dy + dx) sum_footprint |d| + sum w dslack   (+ SHORT U32 (|previous| + |sum|) when accumulated: one add)"""

    def __init__(self, low, t, hd, wd, ignore_index, gs=1.0, exact=False):
        n, hs, ws, classes = low.shape
        self.shape = (n, hs, ws, classes, hd, wd)
        y0, y1, hy, ly = up_axis(hs, hd)
        x0, x1, hx, lx = up_axis(ws, wd)
        self.Wy, self.Wx = _w_matrix(y0, y1, hy, ly, hs), _w_matrix(x0, x1, hx, lx, ws)
        ld_ = low.double()
        T = lambda a: torch.from_numpy(a.astype(np.float64))            # noqa: E731
        a, b = ld_[:, y0][:, :, x0], ld_[:, y0][:, :, x1]
        c, d = ld_[:, y1][:, :, x0], ld_[:, y1][:, :, x1]
        HY, LY = T(hy)[None, :, None, None], T(ly)[None, :, None, None]
        HX, LX = T(hx)[None, None, :, None], T(lx)[None, None, :, None]
        v = HY * (HX * a + LX * b) + LY * (HX * c + LX * d)
        dy, dx = 2 * U32 * (hs + 1), 2 * U32 * (ws + 1)
        self.dw = dy + dx
        if exact:
            f = lambda q: q.float()                                     # noqa: E731
            v32 = f(HY) * (f(HX) * f(a) + f(LX) * f(b)) + f(LY) * (f(HX) * f(c) + f(LX) * f(d))
            assert torch.equal(v32.double(), v), 'not an exact case: the fp32 interpolant differs from the fp64 one'
            err = torch.zeros_like(v)
        else:
            Mw = HY * (HX * a.abs() + LX * b.abs()) + LY * (HX * c.abs() + LX * d.abs())
            Mmax = torch.maximum(torch.maximum(a.abs(), b.abs()), torch.maximum(c.abs(), d.abs()))
            err = 4 * U32 * Mw + 2 * self.dw * Mmax
        self.v = v
        vb = bf(v.float()).double()
        slack = (bf((v + err).float()).double() - bf((v - err).float()).double()).abs()
        self.up = vb.reshape(-1, classes)
        self.ce = CERef(self.up, t.reshape(-1), ignore_index, 0.0, e_exp=E_FEXP, e_log=E_FLOG, adds=8 * cdiv(classes, 8),
                        slack=slack.reshape(-1, classes))
        self.n_slack = self.ce.n_slack
        # backward
        dup, mag, wide = self.ce.grad(gs)
        E = U32 * mag + wide
        self.dup = bf(dup.float()).double()
        dslack = (bf((dup + E).float()).double() - bf((dup - E).float()).double()).abs()
        self.n_dslack = int((dslack > 0).sum())
        sh = (n, hd, wd, classes)
        adj = lambda q, wy, wx: torch.einsum('yY,xX,nyxc->nYXc', wy, wx, q.reshape(sh))      # noqa: E731
        Iy, Ix = (self.Wy > 0).double(), (self.Wx > 0).double()
        self.terms = int(Iy.sum(0).max()) * int(Ix.sum(0).max())
        self.dlow = adj(self.dup, self.Wy, self.Wx)
        self.b_dlow = U32 * (self.terms + 2) * adj(self.dup.abs(), self.Wy, self.Wx) + self.dw * adj(self.dup.abs(), Iy, Ix)
        self.s_dlow = adj(dslack, self.Wy, self.Wx)
        self.unmapped = (Iy.sum(0) == 0)[:, None] | (Ix.sum(0) == 0)[None, :]         # [hs][ws]: no destination maps here

    def check_bwd(self, tag, dlow, prev=None, frac=1.0):
        rec = tag if frac == 1.0 else None
        want, b = self.dlow, frac * self.b_dlow + self.s_dlow
        if prev is not None:
            want = want + prev.double()
            b = b + frac * SHORT * U32 * (prev.double().abs() + want.abs())
        bounded(dlow, want, b, A_BF if frac == 1.0 else 0.0, 1.0, 'dlow' + ('' if prev is None else ' (accumulated)'), rec)


def up_fp32(low, t, hd, wd, ignore_index, wrong=None):
    """the fused operation in plain fp32 with the kernel's two bf16 roundings; lse, row_loss, loss, unrounded dlow.
    wrong = 'swap_y': the weights of the two source rows exchanged"""
    n, hs, ws, classes = low.shape
    y0, y1, hy, ly = up_axis(hs, hd)
    x0, x1, hx, lx = up_axis(ws, wd)
    if wrong == 'swap_y':
        hy, ly = ly, hy
    f = low.float()
    T = torch.from_numpy
    a, b, c, d = f[:, y0][:, :, x0], f[:, y0][:, :, x1], f[:, y1][:, :, x0], f[:, y1][:, :, x1]
    HY, LY, HX, LX = T(hy)[None, :, None, None], T(ly)[None, :, None, None], T(hx)[None, None, :, None], T(lx)[None, None, :, None]
    up = bf(HY * (HX * a + LX * b) + LY * (HX * c + LX * d)).reshape(-1, classes)
    tt = t.reshape(-1)
    l, rl, loss, den = ce_fp32(up, tt, ignore_index, 0.0)
    return up, l, rl, loss, den, (y0, y1, hy, ly, x0, x1, hx, lx)


def up_fp32_bwd(up, t, shape, ignore_index, lse32, den, gs, axes):
    n, hs, ws, classes, hd, wd = shape
    y0, y1, hy, ly, x0, x1, hx, lx = axes
    dup = bf(ce_fp32_bwd(up, t.reshape(-1), ignore_index, 0.0, lse32, den, gs)).float().reshape(n, hd, wd, classes)
    Wy, Wx = _w_matrix(y0, y1, hy, ly, hs).float(), _w_matrix(x0, x1, hx, lx, ws).float()
    return torch.einsum('yY,xX,nyxc->nYXc', Wy, Wx, dup)


# ---- Dice -------------------------------------------------------------------------------------------------------------------------
def dice_rows(rows):
    """restatement of tok_dice_rows: a block of four waves per four rows, at most 2048 blocks"""
    return min(max(cdiv(rows, 4), 1), 2048)


def make_dice(rows, classes, mode, seed, empty_class=None):
    g = torch.Generator().manual_seed(seed)
    z = bf(torch.randn(rows, classes, generator=g) * 2)
    if mode == 0:
        t = torch.randint(0, classes, (rows,), generator=g)
        if empty_class is not None:
            t[t == empty_class] = (empty_class + 1) % classes
    else:
        t = (torch.rand(rows, classes, generator=g) < 0.4).float()
        if empty_class is not None:
            t[:, empty_class] = 0.0
        if mode == 1:
            t = t[:, 0].contiguous()
    return z, t


class DiceRef:
    """p, y per mode; I = sum p y, P = sum p, Y = sum y per class.
    p        softmax: E_EXP + |z - max| on the exponential, six roundings in the 64-lane butterfly, one in the quotient;
             sigmoid 1 / (1 + exp(-z)): E_EXP + 2.  rel_p = the count per element, in units of U32.
    I, P     a lane adds the rows of its wave in sequence, chain = cdiv(rows, 4 grid) fused multiply-adds, the four waves of a
             block add three more; the fold of the partial rows is fp64:  |err| <= U32 sum (rel_p + chain + 3) p y  (p for P)
    Y        exact (an integer below 2^24)
    loss, coef   from the folded sums in fp32; relative errors add up along b = dl_ds ds_dc / ncount: num = 2 I + smooth 2, den 2, in
             -num / (den den) den counts twice and the product and quotient 2 (8), dl_ds = -1 / score 2 + 2 + two divisions (6), the
             product and / ncount 2: K_FIN = 16 (logf's E_LOG is below the two divisions it replaces); references are evaluated
             on the sums they are GIVEN (the kernel's own when checking finalize alone):  relative K_FIN U32 on coef,
             U32 (K_FIN |l_c| + 1) per class on the loss (1 - score cancels to an absolute rounding of 1)"""
    K_FIN = 16.0

    def __init__(self, z, t, mode, rows_grid):
        zd = z.double()
        rows, classes = zd.shape
        self.mode, self.classes, self.rows = mode, classes, rows
        if mode == 0:
            x = zd - zd.max(1, keepdim=True).values
            e = torch.exp(x)
            p = e / e.sum(1, keepdim=True)
            y = torch.zeros_like(zd)
            y.scatter_(1, t[:, None], 1.0)
            rel = E_EXP + x.abs() + 7.0
        else:
            p = torch.sigmoid(zd)
            y = t.double().reshape(rows, classes)
            rel = torch.full_like(zd, E_EXP + 2.0)
        self.p, self.y, self.rel = p, y, rel
        self.chain = cdiv(rows, 4 * rows_grid)
        k = rel + self.chain + 3.0
        self.I, self.P, self.Y = (p * y).sum(0), p.sum(0), y.sum(0)
        self.m_I, self.m_P = (k * p * y).sum(0), (k * p).sum(0)

    def finalize(self, I, P, Y, smooth, eps, log_loss, sel):
        """fp64 loss, coef[2][classes] of the given sums, and the per-class loss terms |l_c| / ncount for the bound"""
        classes = self.classes
        counted = torch.ones(classes, dtype=torch.bool)
        ncount = classes
        if sel is not None:
            counted = torch.zeros(classes, dtype=torch.bool)
            counted[sel] = True
            ncount = len(sel)
        act = counted & (Y > 0)
        card = P + Y
        den = card.clamp_min(eps) + smooth
        num = 2 * I + smooth
        score = num / den
        if log_loss:
            l, dl = -torch.log(score.clamp_min(eps)), torch.where(score > eps, -1 / score, torch.zeros_like(score))
        else:
            l, dl = 1 - score, -torch.ones_like(score)
        z = torch.zeros_like(score)
        loss = torch.where(act, l, z).sum() / ncount
        m_loss = torch.where(act, self.K_FIN * (l.abs() + score) + 1.0, z).sum() / ncount
        a = torch.where(act, dl * 2 / den / ncount, z)
        b = torch.where(act & (card > eps), dl * (-num / den ** 2) / ncount, z)
        self.num, self.den, self.act, self.log_loss = num, den, act, log_loss
        return loss, m_loss, torch.stack([a, b])

    def coef_rel(self, frac=1.0):
        """relative error of the end-to-end coefficients: num = 2 I + smooth and den = P + Y + smooth carry the errors of I and P;
        a ~ 1 / den (x 1 / score under log_loss), b ~ num / den^2 (x 1 / score)"""
        ri = 2 * frac * U32 * self.m_I.cpu() / self.num.clamp_min(1e-300)
        rp = frac * U32 * self.m_P.cpu() / self.den
        extra = (ri + rp) if self.log_loss else 0.0
        z = torch.zeros_like(ri)
        return torch.stack([torch.where(self.act, rp + extra, z), torch.where(self.act, ri + 2 * rp + extra, z)]) + frac * self.K_FIN * U32

    def grad(self, coef, gs, coef_rel=None):
        """dlogits of the given coef (fp64 of the kernel's own, or the reference's with coef_rel = their relative error);
        magnitude in units of U32.  softmax: p (dp - sum p dp) g, p carries rel_p, the dot product eight roundings more;
        sigmoid: p (1 - p) dp g, where the absolute error of p passes to 1 - p: (rel_p + 6) p |dp g| covers both factors"""
        p, y = self.p, self.y
        dp = coef[0] * y + coef[1]
        ddp = torch.zeros_like(dp) if coef_rel is None else (coef_rel[0] * coef[0].abs() * y + coef_rel[1] * coef[1].abs()) / U32
        if self.mode == 0:
            dot = (p * dp).sum(1, keepdim=True)
            d = p * (dp - dot) * gs
            adot = (p * dp.abs()).sum(1, keepdim=True)
            relmax = self.rel.max(1, keepdim=True).values
            mag = p * ((self.rel + 6.0) * (dp.abs() + adot) + (relmax + 7.0) * adot + ddp + (p * ddp).sum(1, keepdim=True)) * abs(gs)
        else:
            d = p * (1 - p) * dp * gs
            mag = p * ((self.rel + 6.0) * dp.abs() + ddp) * abs(gs) + TAIL / U32 * dp.abs() * abs(gs)
        return d, mag


def dice_fp32(z, t, mode, smooth, eps, log_loss, sel, gs):
    """plain fp32 run: I, P, Y, loss, coef, dlogits (unrounded)"""
    zf = z.float()
    rows, classes = zf.shape
    if mode == 0:
        p = torch.softmax(zf, 1)
        y = torch.zeros_like(zf)
        y.scatter_(1, t[:, None], 1.0)
    else:
        p, y = torch.sigmoid(zf), t.float().reshape(rows, classes)
    I, P, Y = (p * y).sum(0), p.sum(0), y.sum(0)
    counted = torch.ones(classes, dtype=torch.bool)
    ncount = classes
    if sel is not None:
        counted = torch.zeros(classes, dtype=torch.bool)
        counted[sel] = True
        ncount = len(sel)
    act = counted & (Y > 0)
    card = P + Y
    den, num = card.clamp_min(eps) + smooth, 2 * I + smooth
    score = num / den
    if log_loss:
        l, dl = -torch.log(score.clamp_min(eps)), torch.where(score > eps, -1 / score, torch.zeros_like(score))
    else:
        l, dl = 1 - score, -torch.ones_like(score)
    z0 = torch.zeros_like(score)
    loss = torch.where(act, l, z0).sum() / ncount
    coef = torch.stack([torch.where(act, dl * 2 / den / ncount, z0), torch.where(act & (card > eps), dl * (-num / den ** 2) / ncount, z0)])
    dp = coef[0] * y + coef[1]
    d = p * (dp - (p * dp).sum(1, keepdim=True)) * gs if mode == 0 else p * (1 - p) * dp * gs
    return I, P, Y, loss, coef, d


# ---- BCE with logits and an ignore value --------------------------------------------------------------------------------------------
def make_bce(rows, classes, ignore, seed):
    """soft targets in (0, 1), a third of the elements ignored, logits +-90 planted"""
    g = torch.Generator().manual_seed(seed)
    z = bf(torch.randn(rows, classes, generator=g) * 3)
    t = torch.rand(rows, classes, generator=g) * 0.98 + 0.01
    t[torch.rand(rows, classes, generator=g) < 1 / 3] = ignore
    z.view(-1)[0], z.view(-1)[-1] = 90.0, -90.0
    t.view(-1)[0], t.view(-1)[-1] = 0.25, 0.75
    if rows > 2:
        z[1, 0], z[2, classes - 1] = -90.0, 90.0
        t[1, 0], t[2, classes - 1] = 0.0, 1.0
    return z, t


def bce_ref(z, t, ignore, mean, gs):
    """element (1 - t) x - log_sigmoid(x), log_sigmoid(x) = min(x, 0) - log1p(exp(-|x|)): u = exp(-|x|) carries E_EXP, which passes
    to log1p(u) as at most E_EXP u / (1 + u) <= E_EXP log1p(u); log1pf adds E_L1P log1p(u); the product, the two differences and
    1 - t are four roundings of |(1 - t) x| + |x| + log1p(u).  The fold is fp64: loss within one rounding of itself plus the fold
    of the element errors.  Gradient (sigmoid(x) - t) g, g = gscale / n_selected: the sigmoid carries E_EXP + 2, the difference,
    the reciprocal of n, and the two products four more; exp(-x) overflows for x < -88 and the sigmoid is then 0: TAIL.
    Returns loss, its bound, n_selected, dlogits, its magnitude (units of U32)."""
    x, td = z.double(), t.double()
    sel = t != ignore
    u = torch.exp(-x.abs())
    el = (1 - td) * x - (torch.clamp(x, max=0.0) - torch.log1p(u))
    m_el = (E_EXP + E_L1P) * torch.log1p(u) + 4.0 * (((1 - td) * x).abs() + x.abs() + torch.log1p(u))
    n = int(sel.sum())
    zero = torch.zeros_like(el)
    tot, m_tot = torch.where(sel, el, zero).sum(), torch.where(sel, m_el, zero).sum()
    if n == 0:
        loss, b_loss, k = torch.zeros((), dtype=F64), torch.zeros((), dtype=F64), 0.0
    else:
        div = n if mean else 1
        loss, b_loss, k = tot / div, U32 * (tot.abs() + m_tot) / div, abs(gs) / div
    sg = torch.sigmoid(x)
    d = torch.where(sel, (sg - td) * (gs / (n if mean and n else 1)) * (1.0 if n or not mean else 0.0), zero)
    mag = torch.where(sel, ((E_EXP + 2.0) * sg + 4.0 * (sg + td.abs()) + TAIL / U32) * k, zero)
    return loss, b_loss, n, d, mag


def bce_fp32(z, t, ignore, mean, gs):
    x = z.float()
    sel = t != ignore
    el = (1 - t) * x - (torch.clamp(x, max=0.0) - torch.log1p(torch.exp(-x.abs())))
    n = int(sel.sum())
    if n == 0:
        return torch.zeros(()), torch.zeros_like(x)
    tot = el[sel].double().sum()
    g = torch.tensor(gs, dtype=torch.float32) * ((torch.tensor(1.0) / torch.tensor(float(n))) if mean else 1.0)
    return (tot / n if mean else tot).float(), torch.where(sel, (1 / (1 + torch.exp(-x)) - t) * g, torch.zeros(()))


# ---- regression losses --------------------------------------------------------------------------------------------------------------
def make_reg(n, knee, seed):
    """bf16 predictions and fp32 targets; planted where they fit: x - t exactly 0, +-knee, and +-knee +- one bf16 ulp of x (the
    differences are exact in fp32: x is a small bf16 number, t = x - difference)"""
    g = torch.Generator().manual_seed(seed)
    x = bf(torch.randn(n, generator=g) * 2)
    t = torch.randn(n, generator=g) * 2
    ulp = 2.0 ** -7                 # bf16 ulp in [1, 2)
    diffs = [0.0, knee, -knee, knee + ulp, knee - ulp, -knee + ulp, -knee - ulp]
    for i, dlt in enumerate(diffs):
        j = 1 + i
        if j < n:
            x[j] = 1.0 + i * ulp
            t[j] = float(x[j]) - dlt
    return x, t


def _reg_elem(kind, d, k):
    a = d.abs()
    if kind == 0:
        return a, torch.sign(d), a
    if kind == 1:
        return d * d, 2 * d, d * d
    if kind == 2:
        inner = a < k
        return (torch.where(inner, 0.5 * d * d / k, a - 0.5 * k), torch.where(inner, d / k, torch.sign(d)),
                torch.where(inner, d * d / k, a + 0.5 * k))
    inner = a <= k
    return (torch.where(inner, 0.5 * d * d, k * (a - 0.5 * k)), torch.where(inner, d, k * torch.sign(d)),
            torch.where(inner, d * d, k * (a + 0.5 * k)))


def reg_ref(x, t, kind, knee, mean, gs):
    """d = x - t (one rounding), then at most four operations per element (0.5 d d / k): 5 U32 on the magnitude of the
    branch taken (both branches agree in value and slope at the knee, so the rounding of d cannot jump).  The fold is fp64.
    Gradient: d, the element's slope (at most one operation on top of d), 1 / n, gscale * (1 / n) and the product: five roundings,
    SHORT x 5 U32, one bf16 rounding.
    Returns loss, its bound, dx, its magnitude (units of U32)."""
    d = x.double() - t.double()
    el, gr, m_el = _reg_elem(kind, d, float(knee))
    n = d.numel()
    div = n if mean else 1
    loss = el.sum() / div
    b_loss = U32 * (loss.abs() + 5.0 * m_el.sum() / div)
    # the slope's own magnitude: |d| / k inside the knee moves with the rounding of d
    return loss, b_loss, gr * (gs / div), SHORT * 5.0 * gr.abs() * abs(gs) / div


def reg_fp32(x, t, kind, knee, mean, gs, wrong=None):
    d = x.float() - t
    el, gr, _ = _reg_elem(kind, d, float(knee))
    n = d.numel()
    if wrong == 'huber_unit_slope' and kind == 3:
        gr = torch.where(d.abs() <= knee, d, torch.sign(d))
    g = torch.tensor(gs, dtype=torch.float32) * (torch.tensor(1.0) / torch.tensor(float(n)) if mean else 1.0)
    tot = el.double().sum()
    return (tot / n if mean else tot).float(), gr * g


# ---- metric counts ------------------------------------------------------------------------------------------------------------------
def make_counts(rows, classes, ignore_index, seed):
    """bf16 logits with planted ties (columns 5 and 69: one lane's stride; 3 and 40: across lanes; a row of equal columns; a row
    of -inf), int64 predicted labels with out-of-range entries (classes, -1, 2^40 + 1), int64 targets with ignored and out-of-range entries"""
    g = torch.Generator().manual_seed(seed)
    z = bf(torch.randn(rows, classes, generator=g))
    t = torch.randint(0, classes, (rows,), generator=g)
    lab = torch.randint(0, classes, (rows,), generator=g)
    t[torch.rand(rows, generator=g) < 0.15] = ignore_index
    t[1::17] = classes
    t[2::19] = -3
    lab[3::13] = classes
    lab[4::23] = -1
    lab[5::29] = 2 ** 40 + 1            # (truncated to 32 bits it would be class 1)
    for r, cols in ((0, (5, 69)), (1 % rows, (3, 40)), (3 % rows, (40, 3))):
        if all(c < classes for c in cols):
            for c in cols:
                z[r, c] = 7.0
            t[r] = cols[0]
    if rows > 5:
        z[4], z[5] = 0.5, -math.inf
        t[4], t[5] = 0, 0
    if rows > 6:
        z[6] = -math.inf
        t[6] = classes - 1
    return z, lab, t


def counts_ref(pred, t, classes, ignore_index):
    """numpy / bincount: counts [3][classes] = {true positives, predicted, actual} and confusion [target][prediction]; a prediction
    outside [0, classes) is in no column but its row still counts as actual.  pred: labels, or logits (first maximum, as
    torch.argmax: a row of -inf predicts class 0)"""
    t = t.cpu().numpy()
    if pred.dim() == 2:
        pred = pred.float().argmax(1)
    pred = pred.cpu().numpy()
    ok = (t != ignore_index) & (t >= 0) & (t < classes)
    inr = ok & (pred >= 0) & (pred < classes)
    counts = np.zeros((3, classes), dtype=np.int64)
    counts[0] = np.bincount(pred[inr & (pred == t)], minlength=classes)
    counts[1] = np.bincount(pred[inr], minlength=classes)
    counts[2] = np.bincount(t[ok], minlength=classes)
    conf = np.bincount(t[inr] * classes + pred[inr], minlength=classes * classes).reshape(classes, classes)
    return torch.from_numpy(counts), torch.from_numpy(conf)
