"""fp64 reference of the multi-resolution glue (csrc/resample.hip, fuse_sum.hip, neck_resample.hip): bilinear interpolation with align_corners=False, its exact
transpose, and the HRNet fuse sum with its backward.  Plain torch, no GPU needed (every function follows the device of its
operand, so the past-2^31 cases evaluate it on the device from slices).  NHWC throughout: x is [n][h][w][c].

Source index.  `src_index(n_in, n_out)` is ATen's area_pixel_compute_source_index with align_corners=False.  The scale is
the fp32 quotient float(n_in) / float(n_out) — one rounding, and that is the DEFINITION (the kernels and ATen's fp32 path
both start from it).  From it, in fp64,
    s = max(scale (d + 0.5) - 0.5, 0),  i0 = min(int(s), n_in - 1),  i1 = i0 + (i0 < n_in - 1),  lam = s - i0.
The kernels evaluate s in fp32, and hipcc may contract the multiply and the subtraction into one fma.  Three fp32 operations
lie between d and s: (float)d + 0.5 (exact below 2^23, counted all the same), the product with the scale (at most
2^-24 (s + 0.5)) and the subtraction of 0.5 (at most 2^-24 s; none when contracted).  lam = s - i0 is exact (Sterbenz), so
    |d lam| <= K_LAM 2^-24 (s + 1),  K_LAM = 3,
which `src_index` returns beside the indices.  (The rounding of 1 - lam is a relative error of a WEIGHT and belongs to the
accumulation term of a bound, not here.)  At an integer factor 2^k everything above is exact in fp32 and d lam is slack.

What d lam does to a result.  The interpolant is continuous and piecewise linear in s, so moving s by e moves the result by
at most e times the slope of the interval s lies in — |x[i1] - x[i0]| — also when the move carries s across an integer and
the kernel's i0 differs from the reference's: then the slope of the neighbouring interval takes part, and `lam_term`
includes that interval for exactly the destinations whose lam lies within d lam of 0 or 1.  The other axis enters through its
(non-negative) weights.  The transpose has no difference to offer: there a moved weight moves |g| of one destination between
two neighbouring sources, and `lam_term_T` charges d lam |g| to every source the destination can reach.  Terms of second
order (d lam_y d lam_x, below 2^-40 of the data) are left to the slack of K_LAM.
"""
import torch

K_LAM = 3
U32 = 2.0 ** -24


def src_index(n_in, n_out, device=None):
    """(i0, i1, lam, dlam) of every destination index 0 .. n_out - 1: int64, int64, fp64, fp64"""
    scale = (torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)).double().item()
    d = torch.arange(n_out, dtype=torch.float64, device=device)
    s = (scale * (d + 0.5) - 0.5).clamp_min(0.0)
    i0 = s.floor().long().clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    lam = s - i0.double()
    return i0, i1, lam, K_LAM * U32 * (s + 1.0)


def _bc(v, dim):
    shape = [1, 1, 1, 1]
    shape[dim] = -1
    return v.view(shape)


def _up(x, size, rows, absolute):
    n, hs, ws, c = x.shape
    hd, wd = size
    y0, y1, ly, _ = src_index(hs, hd, x.device)
    x0, x1, lx, _ = src_index(ws, wd, x.device)
    if rows is not None:
        y0, y1, ly = y0[rows[0]:rows[1]], y1[rows[0]:rows[1]], ly[rows[0]:rows[1]]
    x = x.double().abs() if absolute else x.double()
    v = x[:, y0] * _bc(1.0 - ly, 1) + x[:, y1] * _bc(ly, 1)
    return v[:, :, x0] * _bc(1.0 - lx, 2) + v[:, :, x1] * _bc(lx, 2)


def up64(x, size, rows=None):
    """separable fp64 interpolation of x [n][hs][ws][c] to size = (hd, wd); rows = (lo, hi) returns destination rows lo .. hi - 1 only"""
    return _up(x, size, rows, False)


def up_mag(x, size, rows=None):
    """up64 of |x|: the magnitude of the interpolation's sum (the weights are non-negative)"""
    return _up(x, size, rows, True)


def _up_T(g, size, absolute):
    n, hd, wd, c = g.shape
    hs, ws = size
    y0, y1, ly, _ = src_index(hs, hd, g.device)
    x0, x1, lx, _ = src_index(ws, wd, g.device)
    g = g.double().abs() if absolute else g.double()
    t = torch.zeros(n, hd, ws, c, dtype=torch.float64, device=g.device)
    t.index_add_(2, x0, g * _bc(1.0 - lx, 2)).index_add_(2, x1, g * _bc(lx, 2))
    out = torch.zeros(n, hs, ws, c, dtype=torch.float64, device=g.device)
    return out.index_add_(1, y0, t * _bc(1.0 - ly, 1)).index_add_(1, y1, t * _bc(ly, 1))


def up64_T(g, size):
    """the exact transpose of up64(., g.shape[1:3]) applied to g [n][hd][wd][c], size = (hs, ws): scattered with index_add_ from
    the same indices and weights (no autograd)"""
    return _up_T(g, size, False)


def up_T_mag(g, size):
    return _up_T(g, size, True)


def up64_T_rows(g, size, rows):
    """source rows rows[0] .. rows[1] - 1 of up64_T(g, size), from the destination rows that carry a weight on them only (the
    past-2^31 cases: g stays where it is, a band of it is widened to fp64)"""
    n, hd, wd, c = g.shape
    hs, ws = size
    wy = weight_matrix(hs, hd)[:, rows[0]:rows[1]]
    used = (wy > 0).any(1).nonzero().view(-1)
    lo, hi = int(used.min()), int(used.max()) + 1
    x0, x1, lx, _ = src_index(ws, wd, g.device)
    band = g[:, lo:hi].double()
    t = torch.zeros(n, hi - lo, ws, c, dtype=torch.float64, device=g.device)
    t.index_add_(2, x0, band * _bc(1.0 - lx, 2)).index_add_(2, x1, band * _bc(lx, 2))
    return torch.einsum('da,ndbc->nabc', wy[lo:hi].to(g.device), t)


def taps_T(n_in, n_out):
    """the largest number of destinations with a non-zero weight on one source, along one axis (the footprint of the transpose)"""
    i0, i1, lam, _ = src_index(n_in, n_out)
    cnt = torch.zeros(n_in, dtype=torch.int64)
    cnt.index_add_(0, i0, torch.ones_like(i0))                      # 1 - lam > 0 always
    cnt.index_add_(0, i1, ((lam > 0) & (i1 != i0)).long())
    return int(cnt.max())


def weight_matrix(n_in, n_out):
    """W [n_out][n_in] of one axis (fp64): row d holds 1 - lam at i0 and lam at i1 (their sum where i0 == i1)"""
    i0, i1, lam, _ = src_index(n_in, n_out)
    w = torch.zeros(n_out, n_in, dtype=torch.float64)
    d = torch.arange(n_out)
    w.index_put_((d, i0), 1.0 - lam, accumulate=True)
    w.index_put_((d, i1), lam, accumulate=True)
    return w


def _reach(n_in, n_out):
    """(lo, hi, dlam): the sources i with lo <= i <= hi are those a destination can touch once s moves by dlam: i0 .. i1, one
    more below where lam < dlam, one more above where lam > 1 - dlam"""
    i0, i1, lam, dlam = src_index(n_in, n_out)
    lo = (i0 - (lam < dlam).long()).clamp_min(0)
    hi = (i1 + (lam > 1.0 - dlam).long()).clamp_max(n_in - 1)
    return lo, hi, dlam


def slope_matrix(n_in, n_out):
    """S [n_out][max(n_in - 1, 0)]: dlam on the intervals (j, j + 1) whose slope a moved s can take part in"""
    lo, hi, dlam = _reach(n_in, n_out)
    j = torch.arange(max(n_in - 1, 0))
    return ((j[None, :] >= lo[:, None]) & (j[None, :] + 1 <= hi[:, None])).double() * dlam[:, None]


def reach_matrix(n_in, n_out):
    """E [n_out][n_in]: dlam on every source the destination can touch"""
    lo, hi, dlam = _reach(n_in, n_out)
    i = torch.arange(n_in)
    return ((i[None, :] >= lo[:, None]) & (i[None, :] <= hi[:, None])).double() * dlam[:, None]


def lam_term(x, size):
    """absolute bound on what the fp32 evaluation of s does to up64(x, size) (module docstring); x on the host"""
    n, hs, ws, c = x.shape
    hd, wd = size
    x = x.double().cpu()
    wy, wx = weight_matrix(hs, hd), weight_matrix(ws, wd)
    dy, dx = (x[:, 1:] - x[:, :-1]).abs(), (x[:, :, 1:] - x[:, :, :-1]).abs()
    ty = torch.einsum('da,nabc,eb->ndec', slope_matrix(hs, hd), dy, wx)
    tx = torch.einsum('da,nabc,eb->ndec', wy, dx, slope_matrix(ws, wd))
    return ty + tx


def lam_term_T(g, size):
    """the same for up64_T(g, size): d lam |g| of every destination a source is within reach of"""
    n, hd, wd, c = g.shape
    hs, ws = size
    g = g.double().abs().cpu()
    wy, wx = weight_matrix(hs, hd), weight_matrix(ws, wd)
    ty = torch.einsum('da,ndec,eb->nabc', reach_matrix(hs, hd), g, wx)
    tx = torch.einsum('da,ndec,eb->nabc', wy, g, reach_matrix(ws, wd))
    return ty + tx


def dyadic(n_in, n_out):
    """an integer factor 2^k (k >= 0): s, lam and every weight are multiples of 1 / (2 factor), exact in fp32"""
    f = n_out // n_in
    return n_in * f == n_out and f & (f - 1) == 0


# ---- HRNet fuse sum -------------------------------------------------------------------------------------------------------------
def _rep(v, s):
    """nearest-neighbour upsampling by 2^s of [n][h][w][c]: index d reads d >> s"""
    if s == 0:
        return v
    n, h, w, c = v.shape
    iy, ix = torch.arange(h << s) >> s, torch.arange(w << s) >> s
    return v[:, iy][:, :, ix]


def fuse64(terms, shifts, scales, shifts_f, relu, absolute=False):
    """y = relu?(sum_j repeat_{2^s_j}(t_j sc_j + sf_j)) in fp64; sc_j / sf_j are [c] or None (the term as stored).  With
    `absolute` the same sum over absolute values (the magnitude of the accumulation, no relu)."""
    y = None
    for t, s, sc, sf in zip(terms, shifts, scales, shifts_f):
        v = t.double().cpu()
        if absolute:
            v = v.abs()
        if sc is not None:
            v = v * (sc.double().abs() if absolute else sc.double()) + (sf.double().abs() if absolute else sf.double())
        v = _rep(v, s)
        y = v if y is None else y + v
    return y.clamp_min(0.0) if relu and not absolute else y


def fuse_mask(y_bf16):
    """the mask of the stored sum: bit e of byte [pixel][c / 8] is y[pixel][8 byte + e] > 0 (helpers.pack_bits)"""
    from helpers import pack_bits
    c = y_bf16.shape[-1]
    return pack_bits((y_bf16.float() > 0).reshape(-1, c))


def fuse_T64(dout, keep, shift, prev=None, absolute=False):
    """d term = (prev +) the sum over every 2^shift x 2^shift block of (keep ? dout : 0); keep is a bool tensor like dout or None"""
    g = dout.double().cpu()
    if absolute:
        g = g.abs()
    if keep is not None:
        g = torch.where(keep, g, torch.zeros_like(g))
    n, h, w, c = g.shape
    f = 1 << shift
    out = g.view(n, h // f, f, w // f, f, c).sum(dim=(2, 4))
    if prev is not None:
        out = out + (prev.double().cpu().abs() if absolute else prev.double().cpu())
    return out
