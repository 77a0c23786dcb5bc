"""fp64 references of the fused MLP (csrc/mlp_fused.hip: tok_mlp_fwd, tok_mlp_bwd_dx, tok_mlp_serves), of the activation pair of
csrc/layernorm.hip (tok_act_fwd, tok_act_bwd) and of the exact index kernels of csrc/transformer.hip (tok_cpb_bias_fwd / _bwd,
tok_patch_merge) and csrc/vit_embed.hip (tok_patch_gather, tok_vit_embed_fwd / _bwd, tok_rows_select); the bounds of their contracts,
the input makers, the case lists, restatements of the launchers' rules and plain fp32 runs of the same formulas
(tests/test_mlp_rows_ref.py: every reference equals torch's own operation and autograd in fp64, an fp32 run stays inside HALF of the
non-rounding part of every bound, deliberately wrong variants do not pass).  Plain torch / numpy, no HIP.

Every check is |mine - ref| <= bound per element; `bound` is written as a tensor so that the same check serves every output.
U32 = 2^-24 is the fp32 unit roundoff, A_BF = 2^-8 that of bf16 (one rounding to nearest; a result half way between two bf16 values
just above a power of two uses all of it, so ratios of 0.9 - 1.0 on a bf16 output are that rounding).  Products of two bf16 values are
exact in fp32, so a dot product of length K costs its K additions; `mag` is the same product on absolute values.

Fused MLP, stage by stage and each stage from the rows the KERNEL stored for the stage before, so one rounding per bound:
  pre    x W1^T + b1: K = c additions in the MFMA accumulators (any order), the bias add, one bf16 rounding:
         A_BF |ref| + 2 (K + 2) U32 mag, mag = |x| |W1|^T + |b1|.
  act    GELU of the kernel's own pre rows: the GELU bound below.
  y      act_own W2^T + b2: the same form with K = hidden.
  dpre   t = dy W2_dgrad (K = c), rounded to bf16, times GELU'(pre), rounded to bf16:
         2 A_BF |ref| + |g'| 2 (K + 2) U32 mag_t + |t| G_ABS max(1, |pre|): the two roundings, the accumulation of t carried
         through the product, and the GELU' allowance.
  dx     dpre_own W1_dgrad (+ prior), K = hidden: A_BF |ref| + 2 (K + 3) U32 (mag + |prior|).
GELU and GELU' (tok_common.h: a degree-5 polynomial of log2 Phi(-a) under one v_exp_f32, a = min(|x|, 5.6); the header documents
|error in Phi| <= 3e-7): per element A_BF |ref| for the one bf16 rounding of the result and G_ABS max(1, |x|), G_ABS = 2^-20: absolute
slack for the tail approximation, 3 x the documented 3e-7 and 1 / 2048 of the bf16 step of a unit activation (GELU = x Phi(x) and
GELU' = Phi + x phi carry the error of Phi times max(1, |x|)).  tok_act_bwd: dx = bf16(g d(x) + prev):
A_BF |ref| + |g| G_ABS max(1, |x|) + 2 U32 (|g d| + |prev|); ReLU' and the identity are exact, so kinds 0 and 2 get no G_ABS term.
cpb bias   16 sigmoid(t): expf, the add, the division: 4 U32 |ref|.  Backward: the ordered sum of the cnt positions that hit a table
           row, the sigmoid chain (4 roundings) and one bf16 rounding: A_BF |ref| + 2 (cnt + 4) U32 16 s (1 - s) sum |dbias|
           (not modelled: the cancellation in 1 - s for large positive table values, see cpb_cancel).
vit_embed  one fp32 add and one bf16 rounding: A_BF |ref| + U32 (|patch| + |pos|).  Backward: B sequential adds (and the prior):
           2 (B + 1) U32 sum |dout| (+ U32 |prior|), fp32 outputs.
patch merge, patch gather, rows_select (dir 0, dir 1 fresh): permutations, bit-exact.  rows_select dir 1 accumulated: the sum of two bf16
values in fp32 and one bf16 rounding: A_BF |ref| (+ 2 U32 of the magnitude for the fp32 add).

Wrap cases of the MLP (more than 256 tiles: a workgroup walks tiles blockIdx.x, blockIdx.x + 256, ...): the rows are periodic with the
prime period P = 331, x[r] = base[r % P], so the first P rows are checked against fp64 and every other row r must have the bits of row
r % P: a row's result does not depend on which lane or tile computes it, because each element has the same accumulation order."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from helpers import A_BF, BF, F32, U32, cdiv
from loss_ref import bounded, flush_record  # noqa: F401  (used by the test modules)

F64 = torch.float64
G_ABS = 2.0 ** -20
P = 331
GELU_AMAX = 5.6
INV_SQRT2 = 0.7071067811865476
INV_SQRT2PI = 0.3989422804014327


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bf(t):
    return t.to(BF)


def check(tag, what, mine, ref, bound):
    """|mine - ref| <= bound on EVERY element; the worst ratio of (tag, what) is kept for the parity record"""
    return bounded(mine, ref, bound, 0.0, 1.0, what, tag)


# ---- the launcher's rules, restated ---------------------------------------------------------------------------------------------
WIDTHS = (96, 192, 384)
TILE = {96: 256, 192: 256, 384: 128}          # WAVES * NT * 16 of the forms launch_c picks
GRID_CAP = 256                                # mlp_min_blocks is 1 for the 8-wave forms


def mlp_tiles(rows, c):
    return cdiv(rows, TILE[c])


def mlp_serves(rows, c, hidden, min_rows=1):
    """tok_mlp_serves: the hidden rows of every WHOLE tile below 2^32 bytes (32-bit byte offsets for every row of the last tile)"""
    return int(c in WIDTHS and hidden == 4 * c and rows >= max(min_rows, 1) and mlp_tiles(rows, c) * TILE[c] * hidden * 2 < 2 ** 32)


def mlp_class(rows, c):
    t = mlp_tiles(rows, c)
    if t > GRID_CAP:
        return 'wrap'
    if t > 1:
        return 'several workgroups' if rows % TILE[c] != 1 else 'one row past a tile'
    return 'one full tile' if rows == TILE[c] else 'a single row' if rows == 1 else 'part of a tile'


def mlp_cases():
    """(rows, c, launch class)"""
    out = []
    for c in WIDTHS:
        t = TILE[c]
        out += [(1, c, 'a single row'), (77, c, 'part of a tile'), (t, c, 'one full tile'), (t + 1, c, 'one row past a tile'),
                (3 * t + 37, c, 'several workgroups'), (256 * t + t + 77, c, 'wrap')]
    return out


MLP_CASES = mlp_cases()
assert [r for r, c, k in MLP_CASES if k == 'wrap'] == [65869, 65869, 32973]


def act_blocks(count):
    return min(cdiv(count // 8, 256), 65536)


ACT_TRIP = 65536 * 256 * 8                    # elements one trip of the capped activation grid covers


# ---- GELU -------------------------------------------------------------------------------------------------------------------------
def gelu(x, dt=F64):
    x = x.to(dt)
    return 0.5 * x * (1.0 + torch.erf(x * INV_SQRT2))


def gelu_d(x, dt=F64):
    """Phi(x) + x phi(x)"""
    x = x.to(dt)
    return 0.5 * (1.0 + torch.erf(x * INV_SQRT2)) + x * INV_SQRT2PI * torch.exp(-0.5 * x * x)


def gelu_tanh(x, dt=F64):
    """the WRONG activation (the tanh approximation): must not pass the GELU bound"""
    x = x.to(dt)
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def gelu_slack(x):
    return G_ABS * x.double().abs().clamp_min(1.0)


def gelu_bound(x, ref):
    return A_BF * ref.abs() + gelu_slack(x)


_C5 = [np.float32(v) for v in (-1.0000008344650269, -1.1510831117630005, -0.45927679538726807, -0.05253789573907852,
                               0.007387148682028055, -0.0005188509239815176)]


def _tail_np(a):
    """Phi(-a) as tok_common.h has it, with fp32 roundings after every step (an fma rounds once: these round twice, which only
    adds error), numpy's exp2 for v_exp_f32"""
    a = a.astype(np.float32)
    q = a * _C5[5] + _C5[4]
    for k in (3, 2, 1, 0):
        q = (q * a + _C5[k]).astype(np.float32)
    return np.exp2(q).astype(np.float32)


def gelu_poly(x):
    """the polynomial GELU of tok_common.h restated in numpy fp32, before the bf16 rounding (finite inputs)"""
    x = x.float().numpy()
    a = np.minimum(np.abs(x), np.float32(GELU_AMAX)).astype(np.float32)
    m = np.maximum(x, np.float32(0))
    return torch.from_numpy((m - a * _tail_np(a)).astype(np.float32))


def gelu_d_poly(x):
    x = x.float().numpy()
    a = np.minimum(np.abs(x), np.float32(GELU_AMAX)).astype(np.float32)
    t = _tail_np(a)
    cdf = np.where(x >= 0, np.float32(1) - t, t).astype(np.float32)
    with np.errstate(over='ignore'):
        pdf = np.exp2((x * x * np.float32(-0.72134752044448170) + np.float32(-1.3257480647361593)).astype(np.float32)).astype(np.float32)
    return torch.from_numpy((x * pdf + cdf).astype(np.float32))


def bf16_table():
    """all 65536 bf16 bit patterns, in bit order"""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)


def act_d(kind, x, dt=F64):
    x = x.to(dt)
    return (x > 0).to(dt) if kind == 0 else gelu_d(x, dt) if kind == 1 else torch.ones_like(x)


def act_fwd_ref(kind, x):
    """-> (ref, bound); ReLU is exact"""
    xd = x.double()
    if kind == 0:
        return xd.clamp_min(0.0), torch.zeros_like(xd)
    ref = gelu(x)
    return ref, gelu_bound(x, ref)


def act_bwd_ref(kind, g, x, prev, dt=F64):
    """-> (ref, bound) of dx = bf16(g d(x) + prev)"""
    gd = g.to(dt) * act_d(kind, x, dt)
    pv = torch.zeros_like(gd) if prev is None else prev.to(dt)
    ref = gd + pv
    bound = A_BF * ref.abs() + 2 * U32 * (gd.abs() + pv.abs())
    if kind == 1:
        bound = bound + g.to(dt).abs() * gelu_slack(x)
    return ref, bound


def act_bwd_slack(kind, g, x, prev):
    """the non-rounding part of act_bwd_ref's bound"""
    gd = g.double() * act_d(kind, x)
    pv = torch.zeros_like(gd) if prev is None else prev.double()
    return 2 * U32 * (gd.abs() + pv.abs()) + (g.double().abs() * gelu_slack(x) if kind == 1 else 0.0)


def make_act_bwd(seed=0):
    """g = +-1, prior random, for the exhaustive x table"""
    g_ = gen(seed)
    g = bf(torch.randint(0, 2, (65536,), generator=g_).float() * 2 - 1)
    prev = bf(torch.randn(65536, generator=g_))
    return g, prev


# ---- fused MLP --------------------------------------------------------------------------------------------------------------------
def _planted(n, g):
    """n values N(0, 0.3^2), a quarter of them drawn from +-{3, 6} (in a fixed interleave, so every 32-wide stage holds some)"""
    v = torch.randn(n, generator=g) * 0.3
    pick = torch.tensor([3.0, -3.0, 6.0, -6.0])
    idx = torch.arange(0, n, 4)
    v[idx] = pick[torch.randint(0, 4, (idx.numel(),), generator=g)]
    return v


def make_mlp(c, n, seed):
    """n base rows of every operand of both directions; weights scaled by fan-in^-1/2; a quarter of the b1 entries (forward) and of the
    columns of the backward's pre rows are offset by +-{3, 6}, so that the pre-activations cross the GELU clamp at +-5.6 and fill the
    negative tail"""
    g = gen(seed)
    h = 4 * c
    d = dict(c=c, h=h, n=n)
    d['x'] = bf(torch.randn(n, c, generator=g))
    d['w1'] = bf(torch.randn(h, c, generator=g) * c ** -0.5)
    d['w2'] = bf(torch.randn(c, h, generator=g) * h ** -0.5)
    d['b1'] = _planted(h, g)
    d['b2'] = torch.randn(c, generator=g) * 0.3
    d['dy'] = bf(torch.randn(n, c, generator=g))
    d['pre'] = bf(torch.randn(n, h, generator=g) * 1.5 + _planted(h, g))
    d['w2d'] = bf(torch.randn(h, c, generator=g) * h ** -0.5)        # fc2's dgrad pack [hidden][c]
    d['w1d'] = bf(torch.randn(c, h, generator=g) * c ** -0.5)        # fc1's dgrad pack [c][hidden]
    d['prior'] = bf(torch.randn(n, c, generator=g))
    return d


def reaches_the_tails(pre):
    p = pre.double()
    return bool((p < -GELU_AMAX).any()) and bool((p > GELU_AMAX).any()) and bool(((p > -4) & (p < -3)).any())


def _lin(x, w, b, dt):
    """x w^T (+ b) and the same on absolute values"""
    xd, wd = x.to(dt), w.to(dt)
    v, m = xd @ wd.t(), xd.abs() @ wd.abs().t()
    if b is not None:
        v, m = v + b.to(dt), m + b.to(dt).abs()
    return v, m


def _acc(k, extra):
    return 2 * (k + extra) * U32


def pre_ref(d, x=None, dt=F64):
    v, m = _lin(d['x'] if x is None else x, d['w1'], d['b1'], dt)
    return v, A_BF * v.abs() + _acc(d['c'], 2) * m


def act_ref(pre_own):
    ref = gelu(pre_own)
    return ref, gelu_bound(pre_own, ref)


def y_ref(d, act_own, dt=F64, b2=True):
    v, m = _lin(act_own, d['w2'], d['b2'] if b2 else None, dt)
    return v, A_BF * v.abs() + _acc(d['h'], 2) * m


def dpre_ref(d, dt=F64):
    t, m = _lin(d['dy'], d['w2d'], None, dt)
    gp = gelu_d(d['pre'], dt)
    ref = t * gp
    slack = gp.abs() * _acc(d['c'], 2) * m + t.abs() * gelu_slack(d['pre']).to(dt)
    return ref, 2 * A_BF * ref.abs() + slack, slack


def dx_ref(d, dpre_own, acc, dt=F64):
    v, m = _lin(dpre_own, d['w1d'], None, dt)
    if acc:
        v, m = v + d['prior'].to(dt), m + d['prior'].to(dt).abs()
    return v, A_BF * v.abs() + _acc(d['h'], 3) * m, _acc(d['h'], 3) * m


def mlp_fp32(d, acc):
    """the kernel's chain in plain fp32 torch with its rounding points (pre and act to bf16; t and dpre to bf16) and F.gelu, BEFORE the
    last rounding of each output: what must stay inside half of the non-rounding part of each bound"""
    pre = d['x'].float() @ d['w1'].float().t() + d['b1']
    pre_own = bf(pre)
    act = F.gelu(pre_own.float())
    act_own = bf(act)
    y = act_own.float() @ d['w2'].float().t() + d['b2']
    t = bf(d['dy'].float() @ d['w2d'].float().t()).float()
    x = d['pre'].float().requires_grad_(True)
    gp, = torch.autograd.grad(F.gelu(x).sum(), x)
    dpre = t * gp
    dpre_own = bf(dpre)
    dx = dpre_own.float() @ d['w1d'].float().t() + (d['prior'].float() if acc else 0.0)
    return dict(pre=pre, pre_own=pre_own, act=act, act_own=act_own, y=y, dpre=dpre, dpre_own=dpre_own, dx=dx)


# ---- SwinV2 continuous position bias --------------------------------------------------------------------------------------------
def swin_index(ws):
    """relative_position_index of a ws x ws window: int64 [ws^2][ws^2], values below (2 ws - 1)^2"""
    co = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing='ij')).flatten(1)
    rel = (co[:, :, None] - co[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


CPB_WS = {4: 'under one trip', 7: 'ragged trip', 8: 'whole trips', 16: 'many trips'}


def cpb_class(ws):
    """the backward walks the ws^4 positions in trips of 64 lanes x 8"""
    nn = ws ** 4
    return 'under one trip' if nn < 512 else 'ragged trip' if nn % 512 else 'whole trips' if nn < 65536 else 'many trips'


CPB_CASES = [(ws, heads) for ws in CPB_WS for heads in (3, 8)]
CPB_LD = 8
CPB_SPARE_ROWS = 5


def make_cpb(ws, heads, seed):
    g = gen(seed)
    index = swin_index(ws)
    n = ws * ws
    rows = (2 * ws - 1) ** 2 + CPB_SPARE_ROWS
    table = bf(torch.randn(rows, heads, generator=g) * 2)
    assert float(table.float().abs().max()) < 8.5          # the range cpb_cancel's estimate is made for
    dbias = torch.randn(heads, n, n, generator=g)
    return dict(index=index, n=n, rows=rows, table=table, dbias=dbias, heads=heads)


def cpb_fwd_ref(table, index, dt=F64):
    """[heads][n][n] = 16 sigmoid(table[index])"""
    n = index.shape[0]
    v = 16.0 * torch.sigmoid(table.to(dt)[index.reshape(-1)]).view(n, n, -1).permute(2, 0, 1).contiguous()
    return v, 4 * U32 * v.abs()


def cpb_bwd_ref(d, transposed, dt=F64, index=None):
    """dtable [rows][heads]; transposed: dbias is stored [h][j][i]"""
    index = d['index'] if index is None else index
    db = d['dbias'].to(dt)
    if transposed:
        db = db.transpose(1, 2)
    flat = db.permute(1, 2, 0).reshape(d['n'] ** 2, d['heads'])
    s = torch.zeros(d['rows'], d['heads'], dtype=dt).index_add_(0, index.reshape(-1), flat)
    m = torch.zeros(d['rows'], d['heads'], dtype=dt).index_add_(0, index.reshape(-1), flat.abs())
    cnt = torch.bincount(index.reshape(-1), minlength=d['rows']).to(dt)[:, None]
    sg = torch.sigmoid(d['table'].to(dt))
    k = 16.0 * sg * (1.0 - sg)
    ref = s * k
    slack = 2 * (cnt + 4) * U32 * k * m
    return ref, A_BF * ref.abs() + slack, slack


def cpb_cancel(d, transposed):
    """What the bound of the backward does NOT model: 1 - s is formed in fp32 from s = 1 / (1 + e), whose add and division round
    relative to s, so relative to 1 - s they grow as s nears 1: 2 U32 s / (1 - s), with the rounding of the subtraction and the
    error of expf 4 U32 s / (1 - s) |ref| on the result at most.  It is a relative error of the FACTOR 16 s (1 - s), so it scales with
    |ref|, not with the magnitude.  For the tables here (|t| < 8.5) it stays below 4 e^8.5 U32 = 1.2e-3 |ref|, a third of A_BF |ref|;
    the fp32 restatement is held to half of the accumulation term plus this (tests/test_mlp_rows_ref.py), the kernel to the bound as
    the contract states it (worst measured |err| / bound on an MI355X: 0.993, the bf16 rounding)."""
    assert float(d['table'].float().abs().max()) < 8.5
    sg = torch.sigmoid(d['table'].double())
    return 4 * U32 * sg / (1.0 - sg) * cpb_bwd_ref(d, transposed)[0].abs()


# ---- permutations -----------------------------------------------------------------------------------------------------------------
MERGE_CASES = [(1, 2, 2, 8), (2, 8, 12, 16), (3, 6, 10, 24)]
MERGE_BIG = (2, 514, 512, 256)                # 2 * 514 * 512 * 256 / 8 vectors > 65536 blocks x 256 threads
assert MERGE_BIG[0] * MERGE_BIG[1] * MERGE_BIG[2] * MERGE_BIG[3] // 8 > 65536 * 256


def patch_merge_ref(x, order=(0, 1, 2, 3)):
    """PatchMerging: cat(x0, x1, x2, x3) with x0 = x[:, 0::2, 0::2], x1 = x[:, 1::2, 0::2], x2 = x[:, 0::2, 1::2], x3 = x[:, 1::2, 1::2]"""
    parts = [x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]]
    return torch.cat([parts[i] for i in order], -1)


GATHER_CASES = [(1, 3, 5, 1), (3, 4, 6, 2), (1, 8, 12, 4), (3, 32, 48, 16), (3, 10, 6, 2), (1, 16, 32, 16)]


def patch_gather_ref(img, p):
    """[n][h][w][4] -> [n (h/p) (w/p)][p p 4], element (py, px, ch) of a row at (py p + px) 4 + ch"""
    n, h, w, ch = img.shape
    return img.view(n, h // p, p, w // p, p, ch).permute(0, 1, 3, 2, 4, 5).reshape(n * (h // p) * (w // p), p * p * ch)


def bit_pattern(numel, seed, device='cpu'):
    """bf16 values with distinct-looking bits and no NaN (finite normal range), so that a permutation is checked on bits"""
    g = torch.Generator(device=device).manual_seed(seed)
    return bf(torch.randn(numel, generator=g, device=device) * 4)


# ---- ViT token assembly ---------------------------------------------------------------------------------------------------------
EMBED_B, EMBED_P, EMBED_D = (1, 3), (1, 5, 196), (8, 24, 192)


def make_embed(b, p, d, has_cls, seed):
    g = gen(seed)
    t = p + (1 if has_cls else 0)
    return dict(b=b, p=p, d=d, t=t, patch=bf(torch.randn(b * p, d, generator=g)), pos=torch.randn(t, d, generator=g),
                cls=torch.randn(d, generator=g) if has_cls else None, dout=bf(torch.randn(b * t, d, generator=g)),
                dpos_prior=torch.randn(t, d, generator=g), dcls_prior=torch.randn(d, generator=g))


def embed_fwd_ref(e, nec, dt=F64, shift=0):
    """-> (ref [b][t][d], slack); `shift`: the WRONG position row (off by `shift`) under no_embed_class"""
    b, p, d = e['b'], e['p'], e['d']
    prefix = 0 if e['cls'] is None else 1
    pos, patch = e['pos'].to(dt), e['patch'].to(dt).view(b, p, d)
    rows = torch.arange(p) + (shift if nec else prefix)
    body, mag = patch + pos[rows.clamp(0, e['t'] - 1)], patch.abs() + pos[rows.clamp(0, e['t'] - 1)].abs()
    if prefix:
        c0 = e['cls'].to(dt) + (0.0 if nec else pos[0])
        m0 = e['cls'].to(dt).abs() + (0.0 if nec else pos[0].abs())
        body = torch.cat([c0.expand(b, 1, d), body], 1)
        mag = torch.cat([m0.expand(b, 1, d), mag], 1)
    return body, U32 * mag


def embed_bwd_ref(e, nec, dt=F64):
    """-> (dpos [L][d], dcls [d] or None, slack_pos, slack_cls) without priors; L = patches under no_embed_class, else T"""
    b, t, d = e['b'], e['t'], e['d']
    prefix = 0 if e['cls'] is None else 1
    g = e['dout'].to(dt).view(b, t, d)
    s, m = g.sum(0), g.abs().sum(0)
    k = 2 * (b + 1) * U32
    lo = prefix if nec else 0
    dcls = (s[0], k * m[0]) if prefix else (None, None)
    return s[lo:], dcls[0], k * m[lo:], dcls[1]


SELECT_CASES = [(5, 0, 5), (6, 1, 5), (197, 1, 196), (9, 3, 2), (4, 3, 1)]


def rows_select_ref(src, b, t, first, count, d):
    return src.view(b, t, d)[:, first:first + count].reshape(b * count, d)
