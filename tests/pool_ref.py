"""fp64 references of the pooling kernels (csrc/pool.hip) on NHWC tensors, the bounds their contract tests use, and the shape
lists shared by tests/test_pool_contract_gpu.py (device against these references) and tests/test_pool_ref.py (these references
against ATen on the CPU, so that they are tied to torch and not to a reading of the kernels).

Bounds, as helpers.assert_bounded takes them: |got - ref| <= a |ref| + b mag, `mag` the same operation on absolute values.
  A_BF = 2^-8       one rounding of the result to bf16 (every bf16 output).
  k * U32           k fp32 roundings on the longest path from the inputs to the value that is rounded to bf16:
    max-pool backward   4 U32   at most 4 gradients are summed (3 additions) and `prev` added (1).
    avgpool forward     5 U32   3 additions, the reciprocal 1 / count, the product with it.
    avgpool backward    3 U32   the reciprocal, the product, the addition of `prev`.
    gap backward        3 U32   the reciprocal 1 / hw, the product, the addition of `prev`.
    global-pool bwd     4 U32   the reciprocal 1 / hw, its product with the gradient, the addition of the max part, the
                                addition of `prev` (the products with 0.5 and 1 are exact).
  (hw + 2) * U32    gap / global-pool average: hw - 1 sequential additions, the reciprocal 1 / hw and the product with it
                    (hw + 1 roundings), one more for the second-order terms of the sequential sum.
  (cdiv(m, 256) + 9) * U32   tok_colsum: a thread adds cdiv(m, 256) rows in sequence, the tree over 256 threads adds 8 levels,
                    `accumulate` one more.
  chunk * U32       a row of tok_colsum_partial sums at most `chunk` values, in whatever order: any order of L additions is
                    within (L - 1) U32 sum|x| to first order, and chunk >= L leaves the second order its room.
Mode 2 of the global pool (avgmax) is the chain 0.5 * bf16(bf16(avg) + bf16(max)): three roundings, see avgmax_bound."""
import torch

from helpers import A_BF, U32, cdiv

CAP = 4096 * 256            # threads of the largest grid of pool.hip's grid-stride kernels (grid_for)

MAXPOOL_SHAPES = [(1, 1, 1, 8), (1, 2, 2, 8), (2, 3, 5, 16), (1, 15, 17, 8), (3, 8, 6, 24)]
MAXPOOL_FWD_BIG = (17, 63, 63, 512)          # n P Q c / 8 = 17 * 32 * 32 * 64 > CAP: a second grid-stride trip
MAXPOOL_BWD_BIG = (5, 57, 61, 512)           # n h w c / 8 = 5 * 57 * 61 * 64 > CAP
AVGPOOL_SHAPES = [(n, h, w, c) for h in (1, 2, 5, 8) for w in (1, 2, 7, 8) for c in (8, 24) for n in (1, 3)]
GAP_SHAPES = [(n, hw, c) for hw in (1, 7, 49, 3136) for c in (8, 264) for n in (1, 5)]
GAP_BWD_BIG = (3, 3136, 896)                 # n hw c / 8 = 3 * 3136 * 112 > CAP
COLSUM_SHAPES = [(1, 8, 8), (255, 16, 10), (257, 16, 16), (1000, 1000, 1000)]
PARTIAL_NPAD = [8, 288, 2048, 3072, 16384]
PARTIAL_M = [1, 255, 257, 1000]
PARTIAL_TALL = (262145, 8)                   # 1024 rows of 257: the last blocks own no row


def pooled(n):
    return (n - 1) // 2 + 1                  # 3 / 2 / 1 and 2 / 2 / ceil give the same extent


# ---- 3x3 / stride 2 / pad 1 max-pool -------------------------------------------------------------------------------------
def _tap_rows(extent, out, t):
    i = 2 * torch.arange(out) - 1 + t
    return i.clamp(0, extent - 1), (i >= 0) & (i < extent)


def maxpool_fwd(x):
    """x [n][h][w][c] -> (max fp64 [n][P][Q][c], tap int64 = r * 3 + s).  The taps are scanned in (r, s) order over the
    in-bounds ones; a tap replaces the running maximum when it is greater or NaN (ATen: `val > max || isnan(val)`), so the
    FIRST of equal maxima wins, the LAST NaN wins, and an all -inf window reports its first in-bounds tap."""
    n, h, w, c = x.shape
    P, Q = pooled(h), pooled(w)
    xd = x.double()
    best = torch.full((n, P, Q, c), float('-inf'), dtype=torch.float64)
    tap = torch.full((n, P, Q, c), -1, dtype=torch.int64)
    for r in range(3):
        ih, okh = _tap_rows(h, P, r)
        for s in range(3):
            iw, okw = _tap_rows(w, Q, s)
            v = xd[:, ih][:, :, iw]
            ok = (okh[:, None] & okw[None, :])[None, :, :, None]
            take = ok & ((v > best) | v.isnan() | (tap < 0))
            best = torch.where(take, v, best)
            tap = torch.where(take, torch.tensor(r * 3 + s), tap)
    return best, tap


def maxpool_bwd(dy, tap, h, w, prev=None):
    """fp64 scatter: dx[n][2p - 1 + r][2q - 1 + s][c] = prev + sum of dy[n][p][q][c] over the windows whose tap is (r, s)"""
    n, P, Q, c = dy.shape
    dx = torch.zeros(n, h, w, c, dtype=torch.float64) if prev is None else prev.double().clone()
    g = dy.double()
    for r in range(3):
        p0 = 1 if r == 0 else 0                                  # first window whose row 2p - 1 + r is inside
        p1 = min(P, (h - r) // 2 + 1)                            # 2p - 1 + r <= h - 1
        for s in range(3):
            q0 = 1 if s == 0 else 0
            q1 = min(Q, (w - s) // 2 + 1)
            if p1 <= p0 or q1 <= q0:
                continue
            part = torch.where(tap[:, p0:p1, q0:q1] == r * 3 + s, g[:, p0:p1, q0:q1], torch.zeros((), dtype=torch.float64))
            dx[:, 2 * p0 - 1 + r:2 * p1 - 2 + r:2, 2 * q0 - 1 + s:2 * q1 - 2 + s:2] += part
    return dx


def tap_from_flat(index, h, w):
    """F.max_pool2d's flat index ih * w + iw (NCHW [n][c][P][Q]) -> tap r * 3 + s, NHWC"""
    n, c, P, Q = index.shape
    ih, iw = index // w, index % w
    r = ih - (2 * torch.arange(P).view(1, 1, P, 1) - 1)
    s = iw - (2 * torch.arange(Q).view(1, 1, 1, Q) - 1)
    return (r * 3 + s).permute(0, 2, 3, 1).contiguous()


# ---- AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False) ----------------------------------------------------------------
def _avg_count(h, w):
    ones = torch.zeros(2 * pooled(h), 2 * pooled(w), dtype=torch.float64)
    ones[:h, :w] = 1
    return ones.view(pooled(h), 2, pooled(w), 2).sum((1, 3))


def avgpool_fwd(x):
    n, h, w, c = x.shape
    P, Q = pooled(h), pooled(w)
    xp = torch.zeros(n, 2 * P, 2 * Q, c, dtype=torch.float64)
    xp[:, :h, :w] = x.double()
    return xp.view(n, P, 2, Q, 2, c).sum((2, 4)) / _avg_count(h, w)[None, :, :, None]


def avgpool_bwd(dy, h, w, prev=None):
    g = (dy.double() / _avg_count(h, w)[None, :, :, None]).repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :h, :w]
    return g if prev is None else g + prev.double()


# ---- global pools: x [n][hw][c] ------------------------------------------------------------------------------------------------
def gap_fwd(x):
    return x.double().mean(1)


def gap_bwd(dy, hw, prev=None):
    g = (dy.double() / hw)[:, None, :].expand(-1, hw, -1)
    return g if prev is None else g + prev.double()


def global_max(x):
    """(max fp64 [n][c], argmax int64 [n][c]): the first maximal pixel; with a NaN in the channel the LAST NaN (ATen's
    adaptive_max_pool2d takes `val > max || isnan(val)`); an all -inf channel reports pixel 0"""
    n, hw, c = x.shape
    xd = x.double()
    idx = torch.arange(hw).view(1, hw, 1)
    nan = xd.isnan()
    clean = torch.where(nan, torch.tensor(float('-inf'), dtype=torch.float64), xd)
    mx = clean.amax(1)
    first = torch.where(clean == mx[:, None, :], idx, torch.tensor(hw)).amin(1)
    last_nan = torch.where(nan, idx, torch.tensor(-1)).amax(1)
    has_nan = nan.any(1)
    return torch.where(has_nan, torch.tensor(float('nan'), dtype=torch.float64), mx), torch.where(has_nan, last_nan, first)


def avgmax_ref(x):
    """0.5 * (avg + max) in fp64"""
    return 0.5 * (gap_fwd(x) + global_max(x)[0])


def avgmax_bound(x):
    """The device forms 0.5 * bf16(bf16(avg) + bf16(max)).  max is exact.  e1 = A_BF |avg| + (hw + 2) U32 mean|x| bounds
    bf16(avg) (the gap bound).  s = bf16(avg) + max is rounded to fp32 and then to bf16: (U32 + A_BF) |s|, and
    |s| <= |avg + max| + e1.  The halving and the last conversion are exact.  So
    |out - ref| <= (A_BF + U32) |ref| + 0.5 (1 + A_BF + U32) e1: returned as (a, rest), checked with b = 1 on `rest`."""
    hw = x.shape[1]
    e1 = A_BF * gap_fwd(x).abs() + (hw + 2) * U32 * x.double().abs().mean(1)
    return A_BF + U32, 0.5 * (1 + A_BF + U32) * e1


def global_pool_bwd(dy, argmax, hw, mode, prev=None):
    """dy [n][>= c or 2c] (mode 3: [avg gradient | max gradient]), argmax [n][c] -> dx fp64 [n][hw][c]; and the same on
    absolute values (the magnitude of the bound)"""
    n, c = argmax.shape
    g = dy.double()
    ga, gm = (g[:, :c], g[:, c:2 * c]) if mode == 3 else (g[:, :c], g[:, :c])
    wa = {1: 0.0, 2: 0.5 / hw, 3: 1.0 / hw}[mode]
    wm = 0.5 if mode == 2 else 1.0
    hit = (torch.arange(hw).view(1, hw, 1) == argmax[:, None, :]).double()
    dx = (ga * wa)[:, None, :] + hit * (gm * wm)[:, None, :]
    mag = (ga.abs() * wa)[:, None, :] + hit * (gm.abs() * wm)[:, None, :]
    if prev is not None:
        dx, mag = dx + prev.double(), mag + prev.double().abs()
    return dx, mag


# ---- column sums ---------------------------------------------------------------------------------------------------------------
def partial_rows(m):
    """tok_colsum_partial_rows, from the header: min(1024, cdiv(m, 256)) rows, each over `chunk` = cdiv(m, rows) rows of dy"""
    g = min(1024, max(1, cdiv(m, 256)))
    return g, cdiv(m, g)


def colsum_partial(x, g, chunk):
    """x [m][n_pad] -> fp64 [g][n_pad] and the same on |x|; a block past the last row leaves zeros"""
    m, n_pad = x.shape
    xp = torch.zeros(g * chunk, n_pad, dtype=torch.float64)
    xp[:m] = x.double()
    xp = xp.view(g, chunk, n_pad)
    return xp.sum(1), xp.abs().sum(1)


def partial_launch(n_pad):
    """launch arithmetic of tok_colsum_partial: (column groups, groups per pass, row lanes, idle threads, LDS bytes)"""
    cgs = n_pad // 8
    cgt = min(cgs, 256)
    rpb = 256 // cgt
    return cgs, cgt, rpb, 256 - cgt * rpb, rpb * n_pad * 4


# ---- inputs shared by the device tests and the CPU tests of this module ---------------------------------------------------------
BF = torch.bfloat16
FAMILIES = ('ties', 'neginf', 'nan')


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(v) * p for v, p in zip(key, (1, 131, 17, 7, 3, 1009))) & 0x7fffffff)


def maxpool_input(shape, family, seed=0):
    """'ties': 4 levels, most windows hold equal maxima; 'neginf': the top half of image 0 is -inf (whole windows see nothing
    else); 'nan': reals with one NaN in five (many windows hold several)"""
    n, h, w, c = shape
    g = _gen(n, h, w, c, seed, FAMILIES.index(family))
    if family == 'nan':
        x = torch.randn(shape, generator=g)
        x[torch.rand(shape, generator=g) < 0.2] = float('nan')
        return x.to(BF)
    x = torch.randint(0, 4, shape, generator=g).float() - 1.5
    if family == 'neginf':
        x[0, :max(2, (h + 1) // 2)] = float('-inf')                 # rows -1..1 of window row 0 at the least
    return x.to(BF)


def global_input(n, hw, c, family, seed=0):
    """x [n][hw][c]: 'ties' 4 levels; 'neginf' channel 0 of image 0 all -inf; 'nan' reals with one NaN in five"""
    g = _gen(n, hw, c, seed, FAMILIES.index(family), 5)
    if family == 'nan':
        x = torch.randn(n, hw, c, generator=g)
        x[torch.rand(n, hw, c, generator=g) < 0.2] = float('nan')
        return x.to(BF)
    x = torch.randint(0, 4, (n, hw, c), generator=g).float() - 1.5
    if family == 'neginf':
        x[0, :, 0] = float('-inf')
    return x.to(BF)


def avg_exact_input(shape, seed=0):
    """multiples of 4 in [-64, 64]: a window sum is a multiple of 4 of magnitude <= 256 and its quotient by 1, 2 or 4 an
    integer of magnitude <= 64 — every sum and quotient is exact in bf16 (test_pool_ref asserts it)"""
    return (torch.randint(-16, 17, shape, generator=_gen(*shape, seed, 11)) * 4).to(BF)


def avgmax_exact_input(n, hw, c, seed=0):
    """x[j] = k + e[j] with integers |k| <= 8, |e| <= 8 and e[hw - 1 - j] = -e[j]: the pixel sum is hw k exactly, the average
    k, the maximum k + max e, avg + max and its half are integers or half-integers below 32: every value of the chain
    0.5 * bf16(bf16(avg) + bf16(max)) is representable in bf16 (test_pool_ref asserts it)"""
    g = _gen(n, hw, c, seed, 13)
    k = torch.randint(-8, 9, (n, 1, c), generator=g)
    e = torch.randint(-8, 9, (n, hw, c), generator=g)
    e = (e - e.flip(1)).clamp(-8, 8)              # antisymmetric in j, and the clamp keeps it so
    return (k + e).to(BF)
