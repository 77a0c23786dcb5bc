"""fp64 references of the HRNet-OCR entries of csrc/ocr.hip (tok_pix_class_matmul, tok_class_pix_expand, tok_weighted_pool,
tok_softmax_rows_f32 / _bwd_f32, tok_softmax_cols_fwd / _bwd, tok_channel_scale) and of the DaViT entries of csrc/channel_attn.hip
(tok_chan_gram, tok_chan_apply, tok_scale_rows_add, tok_dwconv3x3, tok_dwconv3x3_wgrad), the bounds of their contracts, the input
makers, the case lists and plain fp32 runs of the same formulas (tests/test_ocr_chan_ref.py: every reference equals torch's own
operation and autograd in fp64, the chains reproduce oracle/ocr_ref.py and oracle/davit_ref.py, an fp32 run stays inside HALF of
every bound, deliberately wrong variants do not pass).  Plain torch / numpy, no HIP.

Every formula is written ONCE, as a function of the working dtype: in float64 it is the reference, in float32 the plain fp32 run.
Every formula restates the operation (heads/segmentation/ocr.py as oracle/ocr_ref.py has it: softmax over the pixels, matmul with
the class matrix, softmax over the classes; ChannelAttention.forward, ConvPosEnc and the pre-norm residual as oracle/davit_ref.py
has them), not the kernels' loops.  A backward takes exactly the saved tensors its call is given (p, sim, a_in).

An `Out` (metric_learning_ref.Out) is (ref, a, b): |mine - ref| <= a + b per element, absolute.
  a   A_BF = 2^-8 times the magnitude of the value that is STORED as bf16 (0 for fp32 outputs).  Under `accumulate` that value is
      the total, prior included; the prior itself is read exactly.
  b   U32 = 2^-24 per fp32 rounding on the longest path, times the same operation on absolute values.  A sequential sum of n fused
      multiply-adds counts n, the lane-strided sum K(c) = cdiv(c, 64) + 6 (the 6-step butterfly), a 256-thread tree T(n) =
      cdiv(n, 256) + 8.  The roundings of a short element-wise chain are counted twice (loss_ref.SHORT), and so is every single
      rounding of an exponential's argument.  The last addition of a sum and what follows it (the product with scale, the scale
      folded into the staged matrix, a cast) act on the whole magnitude and are such a chain: a sum of n additions and t more
      operations counts cnt(n, t) = n - 1 + SHORT (1 + t) (with one class or one token there is nothing else).  The add of a prior is
      one more short rounding of |v| + |prior|.  An fp64 fold is 2^-40.
The device functions: every expf gets an argument of at most 0 (v - max), inside the measured [-104, 0] of
profiles/loss_contract_intrinsics.json, or far below it (the planted +80 / -80 rows: loss_ref.TAIL per exponential, the range
measured for the metric-learning module); every logf gets a sum in [1, 64].  Two arguments can exceed 0, both by a rounding
only and both inside expf's other measured range [0, 88]: (1) the chan_gram epilogue exp(g - (mx + log sum)) by a few
U32 |lse|; (2) softmax_cols with scale != 1, where hipcc may contract scale * l - mx into one fma while mx is the maximum of the
ROUNDED products: the largest element's argument is then scale * l - fl(scale * l), within U32 |mx| of 0.  (2) is not in the
issue's list; it needs no new measurement, and the bound below counts the rounding of the product either way.

Derivations (first order; products of two bf16 values are exact in fp32):
pix_class_matmul   scale * sum_c x m: K(c) and the product with scale: b = cnt(K(c), 1) |scale| sum |x m|.  fp32 out, no pad.
class_pix_expand   sum_k w (m scale): k fmas, m scale rounded once per term: b = cnt(k, 1) |scale| sum |w m|; a on the total.
weighted_pool      per chunk at most 512 sequential fmas, the fp64 fold (2^-40), its cast to fp32, the product with scale and
                   the add: b = cnt(min(n, 512), 2) |scale| sum |w x| (+ 2^-40 of it); a on the total.
softmax_rows       p_j = exp(x_j - mx) / s: own exponential E_EXP and the rounding of its argument |x_j - mx|; the same,
                   weighted p_i, through s; k adds; 1 / s and the product (SHORT 2); TAIL for the own term and k TAIL p for the sum.
softmax_rows_bwd   p (dp - <p, dp>): the dot k fmas on D = sum |p dp|, a difference and a product:
                   b = |p| (cnt(k, 0) D + SHORT 2 (|dp| + D)).
softmax_cols_fwd   as softmax_rows over the n pixels with z = scale l: the argument carries the rounding of z and of z - mx
                   (A = |z| + |z - mx|; the rounding of mx itself cancels between an exponential and the sum), the sum T(n).
softmax_cols_bwd   scale p (dp - dot): T(n) D, a difference and two products: b = |scale p| (T(n) D + SHORT 3 (|dp| + D)); a on the total.
channel_scale      x s: one product, SHORT; a on the total.  Pad columns: not computed (see include/tok.h).
chan_gram          G = scale X^T Y: rows_per_image sequential fmas (the zero rows that fill the last 64-token tile add exact
                   zeros) and the product: eG = cnt(rpi, 1) |scale| |X|^T |Y|.
                   mode 1: p_j = exp(g_j - lse), lse = mx + log s: through the logits eG_j + sum_i p_i eG_i; s: sum_i p_i (E_EXP +
                   |g_i - mx|) + 32 adds; log: E_LOG max(1, log s); the sum mx + log s: |lse|; the argument |g_j - lse|; E_EXP; TAIL (1 + 32 p).
                   mode 2: A (G - rowsum(G A)) of the GIVEN A: rs 32 fmas on D = sum |G A| and sum |A| eG; a difference, a product:
                   b = |A| (eG + sum_j |A| eG + U32 (32 D + SHORT 2 (|G| + D))).
chan_apply         32 sequential fmas, M scale rounded once per term: b = cnt(32, 1) |scale| |M| |x|; a = A_BF |ref|.
scale_rows_add     s b, + a, + prior: one SHORT rounding per operation present, each on |s b| + |a| + |prior|; a on the total.
                   With row_scale NULL the result is bf16(fl(fl(b + a) + prior)) bit for bit (no product to contract).
dwconv3x3          bias plus 9 fmas: b = cnt(10, 0) (|bias| + conv(|x|, |w|)); a on the total.
dwconv3x3_wgrad    per block a sequential sum of rows_per_block * w terms, the fp64 fold, its cast and the add of the prior:
                   b = cnt(rpb w, 1) sum |dout x| (+ 2^-40 of it).  fp32 outputs."""
import math

import torch
import torch.nn.functional as F

from helpers import A_BF, BF, F32, U32, cdiv
from loss_ref import E_EXP, E_LOG, SHORT, TAIL, bounded, flush_record  # noqa: F401  (used by the test modules)
from metric_learning_ref import K, Out, check, f32v, gen  # noqa: F401

F64 = torch.float64
FOLD = 2.0 ** -40
HD = 32


def cnt(adds, after):
    """roundings of a sum of `adds` additions followed by `after` more operations: the last addition and everything after it act
    on the whole magnitude and form a short chain (SHORT each); the earlier additions act on partial sums and count once"""
    return adds - 1 + SHORT * (1 + after)


def _softmax(z, dim):
    """exp(z - max) / sum exp(z - max): torch.softmax written out (tests/test_ocr_chan_ref.py: equal to it in fp64), so that the
    fp32 run sums with torch.sum and not with softmax's own sequential column loop"""
    e = torch.exp(z - z.amax(dim, keepdim=True))
    return e / e.sum(dim, keepdim=True)


def T(n):
    """roundings of a 256-thread strided sum of n terms and its 8-step tree"""
    return cdiv(n, 256) + 8


def bf(t):
    return t.to(BF)


def _total(v, b, prior, rounded=True):
    """(+ prior): one more short rounding; a = one bf16 rounding of the total"""
    if prior is not None:
        pd = prior.double()
        b = b + SHORT * U32 * (v.abs() + pd.abs())
        v = v + pd
    return Out(v, a=A_BF * v.abs() if rounded else None, b=b)


def _plus(v, prior, dt):
    return v if prior is None else v + prior.to(dt)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def make_ocr(images, n, k, c, seed):
    """x [b][n][c], m [b][k][c] bf16; w [b][n][k] fp32 weights in [0, 1); prior tensors.  Planted where the shape has room: the
    weights of pixel 0 all zero, the weights of class k - 1 all zero, x[0][0][0] = -0.0"""
    g = gen(seed)
    x = bf(torch.randn(images, n, c, generator=g))
    m = bf(torch.randn(images, k, c, generator=g))
    w = torch.rand(images, n, k, generator=g)
    if n > 1:
        w[:, 0] = 0
    if k > 1:
        w[:, :, k - 1] = 0
    x[0, 0, 0] = -0.0
    return dict(x=x, m=m, w=w, prior_nc=bf(torch.randn(images, n, c, generator=g)), prior_kc=bf(torch.randn(images, k, c, generator=g)))


def make_softmax_rows(rows, k, seed):
    """planted: row 0 one +80 among -80s, row 1 constant, row 2 all -0.0"""
    g = gen(seed)
    x = torch.randn(rows, k, generator=g) * 4
    if k > 1:
        x[0] = -80.0
        x[0, k // 2] = 80.0
    if rows > 1:
        x[1] = 1.25
    if rows > 2:
        x[2] = -0.0
    return x, torch.randn(rows, k, generator=g)


def make_softmax_cols(images, n, k, seed):
    """bf16 logits [b][n][k]; planted: column 0 of image 0 one +80 among -80s, the last column of the last image constant"""
    g = gen(seed)
    l = torch.randn(images, n, k, generator=g) * 3
    if n > 1:
        l[0, :, 0] = -80.0
        l[0, n // 2, 0] = 80.0
    if k > 1:
        l[images - 1, :, k - 1] = 0.5
    l[images - 1, n - 1, k // 2] = -0.0
    return bf(l), torch.randn(images, n, k, generator=g), bf(torch.randn(images, n, k, generator=g))


def make_channel_scale(images, n, c, seed):
    """the gate holds an exact 0 and 1 / 0.7 (Dropout2d at p = 0.3)"""
    g = gen(seed)
    x = bf(torch.randn(images, n, c, generator=g))
    x[0, 0, 0] = -0.0
    s = (torch.rand(images, c, generator=g) < 0.7).float() / 0.7
    s[0, 0], s[images - 1, c - 1] = 0.0, 1 / 0.7
    return x, s, bf(torch.randn(images, n, c, generator=g))


def make_chan(images, rpi, heads, seed, scale=HD ** -0.5):
    """x, y [b][rpi][heads * 32] bf16, M [b * heads][32][32] fp32, dout.  Planted: channel 0 of head 0 of image 0 is a constant
    in x and y that puts the logit G[0][0][0] near 60 at `scale` (above 50)"""
    g = gen(seed)
    c = heads * HD
    x = torch.randn(images, rpi, c, generator=g)
    y = torch.randn(images, rpi, c, generator=g)
    amp = math.sqrt(60.0 / (scale * rpi))
    x[0, :, 0], y[0, :, 0] = amp, amp
    y[images - 1, rpi - 1, c - 1] = -0.0
    m = torch.randn(images * heads, HD, HD, generator=g)
    return bf(x), bf(y), m, bf(torch.randn(images, rpi, c, generator=g))


def make_rows_add(rows, ld, rps, seed):
    """row_scale holds an exact 0 (sample 0) and 1 / 0.7 (sample 1)"""
    g = gen(seed)
    a, b, prior = (bf(torch.randn(rows, ld, generator=g)) for _ in range(3))
    b[0, 0] = -0.0
    rs = None
    if rps:
        rs = (torch.rand(cdiv(rows, rps), generator=g) < 0.7).float() / 0.7
        rs[0] = 0.0
        if len(rs) > 1:
            rs[1] = 1 / 0.7
    return a, b, rs, prior


def make_dwconv(n, h, w, c, seed):
    g = gen(seed)
    x = bf(torch.randn(n, h, w, c, generator=g))
    x[0, 0, 0, 0] = -0.0
    return dict(x=x, wt=torch.randn(c, 9, generator=g) / 3, bias=torch.randn(c, generator=g), dout=bf(torch.randn(n, h, w, c, generator=g)),
                prior=bf(torch.randn(n, h, w, c, generator=g)), prior_dw=torch.randn(c, 9, generator=g), prior_db=torch.randn(c, generator=g))


# ---- OCR ---------------------------------------------------------------------------------------------------------------------------
def pix_class_matmul(x, m, scale, dt=F64):
    """torch.matmul(query, key) of ObjectAttentionBlock: out[b][n][k] = scale sum_c x[b][n][c] m[b][k][c]"""
    return f32v(scale) * torch.matmul(x.to(dt), m.to(dt).transpose(1, 2))


def pix_class_matmul_ref(x, m, scale):
    mag = abs(f32v(scale)) * torch.matmul(x.double().abs(), m.double().abs().transpose(1, 2))
    return Out(pix_class_matmul(x, m, scale), b=U32 * cnt(K(x.shape[-1]), 1) * mag)


def class_pix_expand(w, m, scale, prior=None, dt=F64):
    """torch.matmul(sim_map, value): out[b][n][c] (+)= scale sum_k w[b][n][k] m[b][k][c]"""
    return _plus(torch.matmul(w.to(dt), m.to(dt) * f32v(scale)), prior, dt)


def class_pix_expand_ref(w, m, scale, prior=None):
    mag = abs(f32v(scale)) * torch.matmul(w.double().abs(), m.double().abs())
    return _total(class_pix_expand(w, m, scale), U32 * cnt(w.shape[-1], 1) * mag, prior)


def weighted_pool(w, x, scale, prior=None, dt=F64):
    """torch.matmul(probs, feats) of SpatialGather_Module: out[b][k][c] (+)= scale sum_n w[b][n][k] x[b][n][c]"""
    return _plus(f32v(scale) * torch.matmul(w.to(dt).transpose(1, 2), x.to(dt)), prior, dt)


def weighted_pool_ref(w, x, scale, prior=None):
    mag = abs(f32v(scale)) * torch.matmul(w.double().abs().transpose(1, 2), x.double().abs())
    return _total(weighted_pool(w, x, scale), (U32 * cnt(min(w.shape[1], 512), 2) + FOLD) * mag, prior)


def _softmax_bound(z, p, dim, adds, arg_mag):
    """b of p = softmax(z, dim): see the module docstring (arg_mag: what the rounding of an exponential's argument acts on)"""
    n = z.shape[dim]
    arg = SHORT * arg_mag
    through_sum = (p * (E_EXP + arg)).sum(dim, keepdim=True)
    return U32 * p * (E_EXP + arg + through_sum + adds + SHORT * 2) + TAIL * (1 + n * p)


def softmax_rows(x, dt=F64):
    """F.softmax(sim_map, dim=-1)"""
    return _softmax(x.to(dt), -1)


def softmax_rows_ref(x):
    z, p = x.double(), softmax_rows(x)
    return Out(p, b=_softmax_bound(z, p, -1, x.shape[-1], (z - z.max(-1, keepdim=True).values).abs()))


def softmax_rows_bwd(p, dp, dt=F64):
    """autograd of softmax(dim=-1), of the saved p"""
    pp, d = p.to(dt), dp.to(dt)
    return pp * (d - (pp * d).sum(-1, keepdim=True))


def softmax_rows_bwd_ref(p, dp):
    pa, da = p.double().abs(), dp.double().abs()
    D = (pa * da).sum(-1, keepdim=True)
    return Out(softmax_rows_bwd(p, dp), b=U32 * pa * (cnt(p.shape[-1], 0) * D + SHORT * 2 * (da + D)))


def softmax_cols_fwd(logits, scale, dt=F64):
    """F.softmax(scale * probs, dim=pixels) of spatial_gather, logits [b][n][k]"""
    return _softmax(f32v(scale) * logits.to(dt), 1)


def softmax_cols_fwd_ref(logits, scale):
    z, p = f32v(scale) * logits.double(), softmax_cols_fwd(logits, scale)
    arg = (z - z.max(1, keepdim=True).values).abs() + (z.abs() if f32v(scale) != 1.0 else 0.0)
    return Out(p, b=_softmax_bound(z, p, 1, T(z.shape[1]), arg))


def softmax_cols_bwd(p, dp, scale, prior=None, dt=F64):
    """autograd of softmax(scale * logits, dim=pixels) of the saved p: dlogits (+)= scale p (dp - sum_n p dp)"""
    pp, d = p.to(dt), dp.to(dt)
    return _plus(f32v(scale) * pp * (d - (pp * d).sum(1, keepdim=True)), prior, dt)


def softmax_cols_bwd_ref(p, dp, scale, prior=None):
    pa, da = p.double().abs(), dp.double().abs()
    D = (pa * da).sum(1, keepdim=True)
    b = U32 * abs(f32v(scale)) * pa * (T(p.shape[1]) * D + SHORT * 3 * (da + D))
    return _total(softmax_cols_bwd(p, dp, scale), b, prior)


def channel_scale(x, s, prior=None, dt=F64):
    """Dropout2d: out[b][n][c] (+)= x[b][n][c] s[b][c]"""
    return _plus(x.to(dt) * s.to(dt)[:, None, :], prior, dt)


def channel_scale_ref(x, s, prior=None):
    v = channel_scale(x, s)
    return _total(v, SHORT * U32 * v.abs(), prior)


# ---- DaViT -------------------------------------------------------------------------------------------------------------------------
def _heads(t, dt):
    """[b][n][heads * 32] -> [b][heads][n][32]"""
    b, n, c = t.shape
    return t.to(dt).view(b, n, c // HD, HD).permute(0, 2, 1, 3)


def chan_gram(x, y, scale, mode, a_in=None, dt=F64):
    """(k * scale)^T v per (image, head) over all tokens [b * heads][32][32]; mode 1: .softmax(-1); mode 2: its autograd of the saved A"""
    g = (f32v(scale) * torch.matmul(_heads(x, dt).transpose(-1, -2), _heads(y, dt))).reshape(-1, HD, HD)
    if mode == 1:
        return _softmax(g, -1)
    if mode == 2:
        a = a_in.to(dt)
        return a * (g - (g * a).sum(-1, keepdim=True))
    return g


def chan_gram_ref(x, y, scale, mode, a_in=None):
    g = chan_gram(x, y, scale, 0)
    rpi = x.shape[1]
    eg = U32 * cnt(rpi, 1) * abs(f32v(scale)) * torch.matmul(_heads(x, F64).abs().transpose(-1, -2), _heads(y, F64).abs()).reshape(-1, HD, HD)
    if mode == 0:
        return Out(g, b=eg)
    if mode == 1:
        p = torch.softmax(g, -1)
        mx = g.max(-1, keepdim=True).values
        lse = torch.logsumexp(g, -1, keepdim=True)
        s_err = (p * (E_EXP + SHORT * (g - mx).abs())).sum(-1, keepdim=True) + HD
        rel = eg + (p * eg).sum(-1, keepdim=True) + U32 * (s_err + E_LOG * (lse - mx).clamp_min(1.0) + SHORT * (lse.abs() + (g - lse).abs()) + E_EXP)
        return Out(p, b=p * rel + TAIL * (1 + HD * p))
    a = a_in.double().abs()
    D = (g.abs() * a).sum(-1, keepdim=True)
    b = a * (eg + (a * eg).sum(-1, keepdim=True) + U32 * (HD * D + SHORT * 2 * (g.abs() + D)))
    return Out(chan_gram(x, y, scale, 2, a_in), b=b)


def chan_apply(x, m, transposed, scale, dt=F64):
    """(attn @ q^T)^T: out[n][h*32+i] = scale sum_j M[u][i][j] x[n][h*32+j] (transposed: M[u][j][i]) -> [b][n][heads * 32]"""
    b, n, c = x.shape
    mm = m.to(dt).view(b, c // HD, HD, HD) * f32v(scale)
    o = torch.matmul(_heads(x, dt), mm if transposed else mm.transpose(-1, -2))
    return o.permute(0, 2, 1, 3).reshape(b, n, c)


def chan_apply_ref(x, m, transposed, scale):
    mag = chan_apply(x.double().abs(), m.double().abs(), transposed, abs(f32v(scale)))
    v = chan_apply(x, m, transposed, scale)
    return Out(v, a=A_BF * v.abs(), b=U32 * cnt(HD, 1) * mag)


def _row_scale(rs, rps, rows, dt):
    return rs.to(dt)[torch.arange(rows) // rps][:, None]


def scale_rows_add(a, b, rs, rps, prior=None, dt=F64):
    """x + drop_path(f(x)): out (+)= a + row_scale[row / rps] b; a and row_scale optional"""
    v = b.to(dt) if rs is None else _row_scale(rs, rps, b.shape[0], dt) * b.to(dt)
    if a is not None:
        v = v + a.to(dt)
    return _plus(v, prior, dt)


def scale_rows_add_ref(a, b, rs, rps, prior=None):
    v = scale_rows_add(a, b, rs, rps, prior)
    sb = b.double().abs() if rs is None else _row_scale(rs, rps, b.shape[0], F64).abs() * b.double().abs()
    mag = sb + (0 if a is None else a.double().abs()) + (0 if prior is None else prior.double().abs())
    ops = (rs is not None) + (a is not None) + (prior is not None)
    return Out(v, a=A_BF * v.abs(), b=SHORT * U32 * ops * mag)


def _conv(x, wt, flip):
    """the nine taps of a 3x3 / stride 1 / pad 1 depthwise correlation on NHWC (flip: of the tap-flipped filter)"""
    n, h, w, c = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros_like(x)
    for r in range(3):
        for s in range(3):
            t = 8 - (r * 3 + s) if flip else r * 3 + s
            out = out + xp[:, r:r + h, s:s + w, :] * wt[:, t]
    return out


def dwconv3x3(x, wt, bias, flip, prior=None, dt=F64):
    """ConvPosEnc.proj = nn.Conv2d(dim, dim, 3, 1, 1, groups=dim) on NHWC; flip = 1: its data gradient"""
    v = _conv(x.to(dt), wt.to(dt), flip)
    if bias is not None:
        v = v + bias.to(dt)
    return _plus(v, prior, dt)


def dwconv3x3_ref(x, wt, bias, flip, prior=None):
    mag = _conv(x.double().abs(), wt.double().abs(), flip) + (0 if bias is None else bias.double().abs())
    return _total(dwconv3x3(x, wt, bias, flip), U32 * cnt(10, 0) * mag, prior)


def dwconv3x3_wgrad(x, dout, prior_dw=None, prior_db=None, dt=F64):
    """autograd of that convolution to its weight [c][9] and bias [c]"""
    n, h, w, c = x.shape
    xp, g = F.pad(x.to(dt), (0, 0, 1, 1, 1, 1)), dout.to(dt)
    dw = torch.stack([(xp[:, r:r + h, s:s + w, :] * g).sum((0, 1, 2)) for r in range(3) for s in range(3)], 1)
    return _plus(dw, prior_dw, dt), _plus(g.sum((0, 1, 2)), prior_db, dt)


def wgrad_geometry(n, h):
    """(blocks the workspace is sized for, rows per block, blocks launched) — csrc/channel_attn.hip tok_dwconv3x3_wgrad"""
    sized = min(n * h, 1024)
    rpb = cdiv(n * h, sized)
    return sized, rpb, cdiv(n * h, rpb)


def dwconv3x3_wgrad_ref(x, dout, prior_dw=None, prior_db=None):
    dw, db = dwconv3x3_wgrad(x, dout)
    mw, mb = dwconv3x3_wgrad(x.double().abs(), dout.double().abs())
    cnt_ = U32 * cnt(wgrad_geometry(x.shape[0], x.shape[1])[1] * x.shape[2], 1) + FOLD
    return dict(dw=_total(dw, cnt_ * mw, prior_dw, rounded=False), db=_total(db, cnt_ * mb, prior_db, rounded=False))


# ---- launch classes: restatements of the launchers' rules ---------------------------------------------------------------------------
def grid_class(work, cap):
    """blocks_for: 256 units of work per block, at most `cap` blocks (the kernels stride over the rest)"""
    b = cdiv(work, 256)
    return 'below one block' if work < 256 else 'blocks' if b <= cap else 'second trip'


def lane_class(c):
    return 'below 64' if c < 64 else 'exactly 64' if c == 64 else f'{cdiv(c, 64)} trips'


def tile_class(n, tile):
    """n items in tiles of `tile`"""
    return f'{cdiv(n, tile)} x {tile}, {"ragged" if n % tile else "full"}'


def pcm_class(n, c):
    return f'{grid_class(n * 64, 1024)}, {lane_class(c)}'


def pool_class(n, k, c):
    stage = 32 if c <= 256 else 16
    last = (n - 1) % 512 + 1
    return f'{cdiv(n, 512)} chunk(s), stage {stage} {"ragged" if last % stage else "full"}, {cdiv(k * c, 256)} slot(s)'


IMAGES = 2
#             n, k, c, ldx, ldm, class
PCM_CASES = [(1, 1, 1, 8, 3, 'below one block, below 64'), (5, 19, 63, 64, 72, 'blocks, below 64'), (8, 64, 64, 72, 64, 'blocks, exactly 64'),
             (5, 3, 65, 67, 80, 'blocks, 2 trips'), (8, 19, 129, 136, 129, 'blocks, 3 trips'), (4101, 3, 8, 11, 8, 'second trip, below 64'),
             (5, 64, 256, 256, 264, 'blocks, 4 trips')]
#             n, k, c, ldm, ldo, class of n * cdiv(c, 8) threads
CPE_CASES = [(1, 1, 8, 8, 8, 'below one block'), (5, 19, 20, 24, 24, 'below one block'), (5, 19, 20, 27, 32, 'below one block'),
             (300, 64, 64, 64, 72, 'blocks'), (3, 64, 250, 250, 256, 'below one block'), (4100, 1, 513, 513, 520, 'second trip')]
#            n, k, c, ldx, ldo
WP_CASES = [(1, 3, 20, 24, 24), (31, 3, 20, 20, 24), (32, 3, 20, 24, 20), (33, 3, 20, 24, 24), (512, 3, 20, 24, 24), (513, 3, 20, 24, 24),
            (1100, 3, 20, 24, 24), (40, 2, 264, 264, 272), (5, 3, 85, 88, 88), (5, 4, 64, 64, 64), (5, 1, 257, 257, 264), (33, 20, 512, 512, 512)]
WP_CLASSES = ['1 chunk(s), stage 32 ragged, 1 slot(s)', '1 chunk(s), stage 32 ragged, 1 slot(s)', '1 chunk(s), stage 32 full, 1 slot(s)',
              '1 chunk(s), stage 32 ragged, 1 slot(s)', '1 chunk(s), stage 32 full, 1 slot(s)', '2 chunk(s), stage 32 ragged, 1 slot(s)',
              '3 chunk(s), stage 32 ragged, 1 slot(s)', '1 chunk(s), stage 16 ragged, 3 slot(s)', '1 chunk(s), stage 32 ragged, 1 slot(s)',
              '1 chunk(s), stage 32 ragged, 1 slot(s)', '1 chunk(s), stage 16 ragged, 2 slot(s)', '1 chunk(s), stage 16 ragged, 40 slot(s)']
SR_CASES = [(r, k) for r in (1, 255, 256, 257) for k in (1, 19, 64, 150)] + [(524291, 2)]
#            n, k, ld
SC_CASES = [(1, 1, 1), (1, 19, 24), (255, 19, 19), (256, 19, 24), (257, 64, 64), (257, 64, 72), (1000, 19, 24), (1000, 1, 8)]
SC_SCALES = (1.0, 0.37)
#            n, c, ld, class of n * ld / 8 threads
CS_CASES = [(5, 8, 8, 'below one block'), (37, 20, 24, 'below one block'), (37, 20, 40, 'below one block'), (300, 20, 24, 'blocks'),
            (4100, 513, 520, 'second trip')]
CG_RPI = (1, 63, 64, 65, 200)
CA_RPI = (1, 127, 128, 129, 300)
HEADS = (1, 3)
#             rows, ld, rps, a, acc
SRA_CASES = [(37, 96, 0, 1, 0), (37, 96, 0, 0, 1), (37, 96, 0, 1, 1), (64, 8, 16, 1, 0), (50, 24, 16, 1, 0), (50, 24, 16, 0, 1), (50, 24, 16, 1, 1),
             (8200, 1024, 4100, 1, 0)]
DW_MAPS = ((1, 1), (1, 7), (7, 1), (3, 5), (14, 14))
DW_COLS = ((8, 8), (20, 24), (264, 264))
DW_BIG = (2, 64, 64, 1032, 1032)
#              n, h, w, c, ld, (sized, rows per block, launched)
DWG_CASES = [(2, 3, 5, 20, 24, (6, 1, 6)), (32, 32, 3, 8, 8, (1024, 1, 1024)), (25, 41, 2, 8, 8, (1024, 2, 513)), (2, 7, 7, 264, 264, (14, 1, 14))]
