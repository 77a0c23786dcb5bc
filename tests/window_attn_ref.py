"""fp64 reference of tok_window_attn_fwd / _bwd (include/tok.h; SwinTransformerBlock._attn + WindowAttention.forward of
swin.py, SpatialBlock's WindowAttention of davit.py), written from the contract and independently of fake_backend.py:
roll(-shift) and window_partition are ONE index table (window, token) -> token row, window_reverse its inverse.

  WinRef           forward + autograd backward in fp64 on the bf16 inputs, in chunks of images, with the magnitude terms the
                   contract bounds need (P @ |V|, the logit error Delta of bf16-rounded qn / kn, absolute-value gradients)
  emulate_device   the same operation with the device's rounding points (qn, kn, P, dS to bf16; fp64 otherwise), backward
                   written out by hand: what an exact kernel with those operand formats would return
  check_result     the contract itself, shared by the CPU test of the reference (emulation inside HALF of every bound)
                   and tests/test_window_attn_contract_gpu.py (kernel inside the bound)

The bounds (`frac` scales every one of them; 1 for the kernel, 0.5 for the emulation):
  out     |err| <= 2^-8 |ref| + (2^-7 + expm1(2 Delta_i)) (P @ |V|)          element by element
  lse     |err| <= Delta_i + 2^-18 (1 + |ref|)
  dq, dk, dv   worst token row: |err row| / max(|ref row|, |magnitude row| / 4) < 3e-2
  d(bias) |err| <= sum(b_i (|dS| + P rowsum|dS|)),  b_i = expm1(2 Delta_i) + 2^-14.  With the device's own log-sum-exp the
          recomputed rows still sum to 1, so p' = p (1 + e), |e| <= expm1(2 Delta), gives delta' - delta = sum_j e_j dS_ij and
          dS'_ij - dS_ij = e_ij dS_ij - p'_ij sum_j e_j dS_ij: the row term belongs to the magnitude.  2^-14: fp32 exp2 of
          arguments up to ~2^8 (2^-16 relative) and up to 16 fp32 additions per scratch element, four times over.
          Plus the fp32 term sum(e |dS| + P sum_j e P |dP|), e_ij = 2^-22 (1 + |s_ij| + |lse_i|): about six fp32 roundings of
          quantities as large as the logit and the log-sum-exp stand in the exponent's argument (4 u (|s| + |lse|)), and with
          them a recomputed row no longer sums to 1 exactly: a nearly one-hot row (dS ~ 0) still gets p_hot e |dP_hot|.
          The same term, times |cos| and the scale, is part of the d(logit_scale) bound.
  d(logit_scale)  per head, |err| <= scale (sum b_i (|dS| + P rowsum|dS|) |cos| + (r + 2^-14) sum |dS| cosabs), r = 2^-8 where
          the cosine comes from bf16 operands (cosabs = sum_d |qn| |kn|), 0 on the fp32-operand path; exactly 0 for a clamped head.
  scratch rows, d(logit_scale)   the two envelopes above are sums of absolute values and the gradients are cancelling sums far
          below them, so they are also gated the way dq / dk / dv are, at 3e-2: every (scratch row, head, query) row of d(logits)
          against max(|ref row|, |P (|dP| + P.|dP|) row| / 4), every d(logit_scale) partial and the per-head total against
          max(|ref|, rss / 4), rss = scale sqrt(sum (P (|dP| + P.|dP|) cosabs)^2) (independent term errors add in squares; the
          magnitude of dS without the cancellation of dP - delta: a nearly one-hot row has dS ~ 0 and still an fp32 error of p e |dP|).  The envelopes use
          expm1(2 Delta_i) of each query row, not the case's maximum.
Delta_i = scale_h 2^-8 max_j sum_d |qn_id| |kn_jd| on the MFMA SwinV2 path, 0 on the scalar path (fp32 operands) and in plain
mode (raw bf16 q, k are exact MFMA operands)."""
import math

import torch

from helpers import assert_bounded, record_distance

HD = 32
LN100 = math.log(100.0)
GRAD_GATE = 3e-2          # tests/test_kernels_gpu.py's backward gate, applied per token row here
B_FP32 = 2.0 ** -14


def token_index(h, w, ws, shift):
    """[nW][N] long: row (inside one image) of token t of window `win` after roll(-shift, -shift) + window_partition"""
    nwy, nwx = h // ws, w // ws
    wy = torch.arange(nwy).view(nwy, 1, 1, 1)
    wx = torch.arange(nwx).view(1, nwx, 1, 1)
    iy = torch.arange(ws).view(1, 1, ws, 1)
    ix = torch.arange(ws).view(1, 1, 1, ws)
    oy = (wy * ws + iy + shift) % h           # rolled[y] = x[(y + shift) % H]
    ox = (wx * ws + ix + shift) % w
    return (oy * w + ox).reshape(nwy * nwx, ws * ws)


def shift_mask(h, w, ws, shift):
    """the attn_mask buffer of a shifted SwinTransformerBlock: [nW][N][N], 0 inside a region, -100 across"""
    img = torch.zeros(h, w)
    cnt = 0
    for ys in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for xs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[ys, xs] = cnt
            cnt += 1
    mw = img.reshape(-1)[token_index(h, w, ws, 0)]                  # the mask image is partitioned unrolled
    am = mw.unsqueeze(1) - mw.unsqueeze(2)
    return torch.where(am != 0, -100.0, 0.0).contiguous()


def uses_mfma(ws):
    return ws * ws <= 64


def make_inputs(b, h, w, heads, ws, shift, seed, plain=False, ls0=None, sharp_head=None, ls_mean=2.3):
    """qkv, dout (bf16) and, unless `plain`, logit_scale (ls_mean + 0.1 noise; head 0 = ls0 when given: 5.0 is above the ln 100
    clamp), bias (`sharp_head`: +60 on one key per query, rows nearly one-hot) and the shift mask"""
    c, n = heads * HD, ws * ws
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(b * h * w, 3 * c, generator=g).to(torch.bfloat16)
    dout = torch.randn(b * h * w, c, generator=g).to(torch.bfloat16)
    if plain:
        return qkv, dout, None, None, None
    ls = ls_mean + 0.1 * torch.randn(heads, generator=g)
    if ls0 is not None:
        ls[0] = ls0
    bias = torch.randn(heads, n, n, generator=g)
    if sharp_head is not None:
        bias[sharp_head, torch.arange(n), torch.randperm(n, generator=g)] += 60.0
    return qkv, dout, ls, bias, (shift_mask(h, w, ws, shift) if shift else None)


def _split(xw, heads):
    """[bc][nW][N][3c] -> q, k, v [bc][nW][heads][N][32]"""
    bc, nw, n, _ = xw.shape
    t = xw.view(bc, nw, n, 3, heads, HD).permute(3, 0, 1, 4, 2, 5)
    return t[0], t[1], t[2]


def _to_tokens(t, idx, rows):
    """[bc][nW][heads][N][32] -> [bc][H*W][heads*32] (window_reverse + roll(+shift))"""
    bc, nw, heads, n, _ = t.shape
    res = t.new_empty(bc, rows, heads * HD)
    res[:, idx.reshape(-1)] = t.permute(0, 1, 3, 2, 4).reshape(bc, nw * n, heads * HD)
    return res


class WinRef:
    def __init__(self, qkv, dout, b, h, w, heads, ws, shift, logit_scale=None, bias=None, mask=None, chunk=64, bpw=1):
        """`bpw`: images whose d(logits) / d(logit_scale) share one scratch row (tok_window_attn_bwd_rows = ceil(b / bpw) * nW)"""
        c, n, rows = heads * HD, ws * ws, h * w
        idx = token_index(h, w, ws, shift)
        nw = idx.shape[0]
        plain = logit_scale is None
        self.dims = (b, h, w, heads, ws, shift)
        self.plain, self.mfma = plain, uses_mfma(ws)
        ls = None if plain else logit_scale.double().clone().requires_grad_(True)
        bi = None if plain else bias.double().clone().requires_grad_(True)
        madd = None if mask is None else mask.double()[None, :, None]
        with torch.no_grad():
            scale = torch.full((heads,), HD ** -0.5, dtype=torch.float64) if plain else ls.detach().clamp(max=LN100).exp()
        self.scale = scale
        sc4 = scale.view(1, 1, heads, 1)
        rounded = self.mfma and not plain
        outs, lses, mouts, deltas, grads, mgrads = [], [], [], [], [], []
        self.m_dbias = torch.zeros(heads, n, n, dtype=torch.float64)
        self.m_dbias32 = torch.zeros(heads, n, n, dtype=torch.float64)
        self.m_dls32 = torch.zeros(heads, dtype=torch.float64)
        self.m_dls_a = torch.zeros(heads, dtype=torch.float64)
        self.m_dls_b = torch.zeros(heads, dtype=torch.float64)
        self.delta_max = 0.0
        groups = -(-b // bpw)
        if not plain:       # per scratch row (group of images, window): d(logits), its magnitude, the d(logit_scale) partial
            self.ds_g = torch.zeros(groups, nw, heads, n, n, dtype=torch.float64)
            self.m_ds_g = torch.zeros(groups, nw, heads, n, n, dtype=torch.float64)
            self.dls_g = torch.zeros(groups, nw, heads, dtype=torch.float64)
            self.rss_dls_g = torch.zeros(groups, nw, heads, dtype=torch.float64)       # sum of squares until the end
        for b0 in range(0, b, chunk):
            bc = min(chunk, b - b0)
            x = qkv[b0 * rows:(b0 + bc) * rows].double().view(bc, rows, 3 * c).requires_grad_(True)
            go = dout[b0 * rows:(b0 + bc) * rows].double().view(bc, rows, c)
            q, k, v = _split(x[:, idx], heads)
            if plain:
                qn, kn = q, k
                s = (q @ k.transpose(-2, -1)) * HD ** -0.5
            else:
                qn = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
                kn = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)
                cos = qn @ kn.transpose(-2, -1)
                s = cos * ls.clamp(max=LN100).exp().view(1, 1, heads, 1, 1) + bi[None, None]
            if madd is not None:
                s = s + madd
            p = s.softmax(-1)
            o = p @ v
            tok = _to_tokens(o, idx, rows)
            tok.backward(go)
            with torch.no_grad():
                pd, od, qa, ka, va = p.detach(), o.detach(), qn.detach().abs(), kn.detach().abs(), v.detach().abs()
                gw = _split(torch.cat([go, go, go], -1)[:, idx], heads)[0]            # dO in window layout
                ga = gw.abs()
                cosabs = qa @ ka.transpose(-2, -1)
                delta = (sc4 * 2.0 ** -8 * cosabs.amax(-1)) if rounded else torch.zeros(bc, nw, heads, n, dtype=torch.float64)
                self.delta_max = max(self.delta_max, float(delta.max()))
                outs.append(tok.detach().reshape(bc * rows, c))
                lses.append(torch.logsumexp(s.detach(), -1).reshape(bc * nw * heads, n))
                deltas.append(delta.reshape(bc * nw * heads, n))
                coef = (2.0 ** -7 + torch.expm1(2 * delta)).unsqueeze(-1)
                mouts.append(_to_tokens(coef * (pd @ va), idx, rows).reshape(bc * rows, c))
                # absolute-value gradients (every product of the backward with its factors' magnitudes)
                m_ds = pd * (ga @ va.transpose(-2, -1) + (ga * od.abs()).sum(-1, keepdim=True))
                mdq = sc4.unsqueeze(-1) * (m_ds @ ka)
                mdk = sc4.unsqueeze(-1) * (m_ds.transpose(-2, -1) @ qa)
                if not plain:                    # through F.normalize: d = (dn - n <n, dn>) / |x|
                    qi = 1.0 / q.detach().norm(dim=-1, keepdim=True).clamp_min(1e-12)
                    ki = 1.0 / k.detach().norm(dim=-1, keepdim=True).clamp_min(1e-12)
                    mdq = (mdq + qa * (qa * mdq).sum(-1, keepdim=True)) * qi
                    mdk = (mdk + ka * (ka * mdk).sum(-1, keepdim=True)) * ki
                mdv = pd.transpose(-2, -1) @ ga
                mgrads.append([_to_tokens(t, idx, rows).reshape(bc * rows, c) for t in (mdq, mdk, mdv)])
                grads.append([x.grad[..., i * c:(i + 1) * c].reshape(bc * rows, c) for i in range(3)])
                if not plain:
                    dp = gw @ v.detach().transpose(-2, -1)
                    ds = pd * (dp - (pd * dp).sum(-1, keepdim=True))
                    ex = (torch.expm1(2 * delta) + B_FP32)[..., None]                  # per (image, window, head, query)
                    dsm = ex * (ds.abs() + pd * ds.abs().sum(-1, keepdim=True))
                    gi = torch.arange(b0, b0 + bc) // bpw
                    self.ds_g.index_add_(0, gi, ds)
                    m_dst = pd * (dp.abs() + (pd * dp.abs()).sum(-1, keepdim=True))      # |dS| without its cancellation
                    self.m_ds_g.index_add_(0, gi, m_dst)
                    self.dls_g.index_add_(0, gi, scale.view(1, heads) * (ds * cos.detach()).sum((-2, -1)))
                    self.rss_dls_g.index_add_(0, gi, (scale.view(1, heads, 1, 1) * m_dst * cosabs).square().sum((-2, -1)))
                    # fp32 exponent arguments: p' = p (1 + e), |e_ij| <= 2^-22 (1 + |s_ij| + |lse_i|), rows no longer sum to 1
                    sd = s.detach()
                    e32 = 2.0 ** -22 * (1 + sd.abs() + torch.logsumexp(sd, -1, keepdim=True).abs())
                    ds32 = e32 * ds.abs() + pd * (e32 * pd * dp.abs()).sum(-1, keepdim=True)
                    self.m_dbias += dsm.sum((0, 1))
                    self.m_dbias32 += ds32.sum((0, 1))
                    self.m_dls_a += scale * (dsm * cos.detach().abs()).sum((0, 1, 3, 4))
                    self.m_dls32 += scale * (ds32 * cos.detach().abs()).sum((0, 1, 3, 4))
                    self.m_dls_b += scale * (ds.abs() * cosabs).sum((0, 1, 3, 4))
        self.out, self.lse, self.m_out, self.delta = (torch.cat(t) for t in (outs, lses, mouts, deltas))
        self.grad = [torch.cat([g[i] for g in grads]) for i in range(3)]
        self.m_grad = [torch.cat([g[i] for g in mgrads]) for i in range(3)]
        self.dbias = None if plain else bi.grad.detach()
        self.dls = None if plain else ls.grad.detach()
        self.clamped = None if plain else (logit_scale.double() >= LN100)
        if not plain:
            self.rss_dls = self.rss_dls_g.sum((0, 1)).sqrt()
            self.rss_dls_g = self.rss_dls_g.sqrt()


def _bfr(t):
    return t.to(torch.bfloat16).double()


def emulate_device(qkv, dout, b, h, w, heads, ws, shift, logit_scale=None, bias=None, mask=None, bpw=1):
    """The operation with the MFMA kernels' operand roundings (scalar path: none but the bf16 results) and the device forward's
    log-sum-exp in the backward.  Returns out, lse, dqkv (bf16-rounded, as double), d(bias), d(logit_scale) and the scratch rows
    [R][heads][N][N], [R][heads] of `bpw` images each."""
    c, n, rows = heads * HD, ws * ws, h * w
    idx = token_index(h, w, ws, shift)
    plain, mfma = logit_scale is None, uses_mfma(ws)
    rb = _bfr if mfma else (lambda t: t)
    x = qkv.double().view(b, rows, 3 * c)
    q, k, v = _split(x[:, idx], heads)
    go = _split(torch.cat([dout.double().view(b, rows, c)] * 3, -1)[:, idx], heads)[0]
    if plain:
        scale = torch.full((heads,), HD ** -0.5, dtype=torch.float64)
        qn, kn, qi, ki = q, k, None, None
    else:
        scale = logit_scale.double().clamp(max=LN100).exp()
        qi = 1.0 / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        ki = 1.0 / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        qn, kn = rb(q * qi), rb(k * ki)
    sc5 = scale.view(1, 1, heads, 1, 1)
    cos = qn @ kn.transpose(-2, -1)
    s = cos * sc5
    if bias is not None:
        s = s + bias.double()[None, None]
    if mask is not None:
        s = s + mask.double()[None, :, None]
    lse = torch.logsumexp(s, -1)
    p = (s - lse.unsqueeze(-1)).exp()
    out = _bfr(_to_tokens(rb(p) @ v, idx, rows)).reshape(b * rows, c)
    dp = go @ v.transpose(-2, -1)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    dsb, pb = rb(ds * sc5), rb(p)
    dv = pb.transpose(-2, -1) @ go
    dk = dsb.transpose(-2, -1) @ qn
    dq = dsb @ kn
    if not plain:
        dq = (dq - qn * (qn * dq).sum(-1, keepdim=True)) * qi
        dk = (dk - kn * (kn * dk).sum(-1, keepdim=True)) * ki
    dqkv = _bfr(torch.cat([_to_tokens(t, idx, rows) for t in (dq, dk, dv)], -1)).reshape(b * rows, 3 * c)
    if plain:
        return out, lse.reshape(-1, n), dqkv, None, None, None, None
    dls = torch.where(logit_scale.double() < LN100, scale * (ds * cos).sum((0, 1, 3, 4)), 0.0)
    live = (logit_scale.double() < LN100).double()
    gi, groups, nw = torch.arange(b) // bpw, -(-b // bpw), idx.shape[0]
    scr = torch.zeros(groups, nw, heads, n, n, dtype=torch.float64).index_add_(0, gi, ds)
    part = torch.zeros(groups, nw, heads, dtype=torch.float64).index_add_(0, gi, live * scale * (ds * cos).sum((-2, -1)))
    return out, lse.reshape(-1, n), dqkv, ds.sum((0, 1)), dls, scr.reshape(groups * nw, heads, n, n), part.reshape(groups * nw, heads)


def _rel(err, ref_n, mag_n):
    """worst err / max(|ref|, |magnitude| / 4) (and 2^-24 of the largest magnitude: fp32 flushes e^-100-weighted terms)"""
    den = torch.maximum(torch.maximum(ref_n, mag_n / 4), mag_n.max() * 2.0 ** -24)
    return float(torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, float('inf'), 0.0)).max())


def check_result(tag, ref, out, lse, dqkv, dbias=None, dls=None, scratch=None, part=None, frac=1.0, record=True):
    """the contract of the module docstring; `frac` scales every bound.  Returns {name: err / bound or row error}"""
    b, h, w, heads, ws, shift = ref.dims
    c, n = heads * HD, ws * ws
    rec = tag if record else None
    res = {}
    out, lse, dqkv = out.double().cpu(), lse.double().cpu().reshape(-1, n), dqkv.double().cpu()
    assert torch.isfinite(out).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv).all(), tag
    assert (out - ref.out).norm() / ref.out.norm().clamp_min(1e-300) < 1e-2, tag         # the whole-tensor gate, kept
    res['out'] = assert_bounded(out, ref.out, ref.m_out, frac * 2.0 ** -8, frac, 'out', rec)
    res['lse'] = assert_bounded(lse, ref.lse, ref.delta + 2.0 ** -18 * (1 + ref.lse.abs()), 0.0, frac, 'lse', rec)
    for i, what in enumerate(('dq', 'dk', 'dv')):
        mine, want, mag = dqkv[:, i * c:(i + 1) * c], ref.grad[i], ref.m_grad[i]
        # (plus 2^-24 of the largest magnitude row: a row of -100-masked terms underflows in fp32)
        den = torch.maximum(torch.maximum(want.norm(dim=1), mag.norm(dim=1) / 4), mag.norm(dim=1).max() * 2.0 ** -24)
        e = (mine - want).norm(dim=1)
        worst = float(torch.where(den > 0, e / den.clamp_min(1e-300), torch.where(e > 0, float('inf'), 0.0)).max())
        if record:
            record_distance(tag, what, row_rel_err=worst)
        assert worst < frac * GRAD_GATE, (tag, what, worst)
        res[what] = worst
    if ref.plain:
        return res
    # (elements behind the -100 mask carry e^-100-weighted terms: fp32 flushes them, so the magnitude has a floor of 2^-24 of
    # its largest element, as the rows of dq / dk / dv above)
    m_dbias = ref.m_dbias.clamp_min(float(ref.m_dbias.max()) * 2.0 ** -24) + ref.m_dbias32
    res['dbias'] = assert_bounded(dbias, ref.dbias, m_dbias, 0.0, frac, 'dbias', rec)
    r = 2.0 ** -8 if ref.mfma else 0.0
    res['dls'] = assert_bounded(dls, ref.dls, ref.m_dls_a + (r + B_FP32) * ref.m_dls_b + ref.m_dls32, 0.0, frac, 'dlogit_scale', rec)
    assert (ref.dls[ref.clamped] == 0).all()
    dls = dls.double().cpu()
    assert (dls[ref.clamped] == 0).all(), (tag, 'a clamped head has a logit-scale gradient')
    # the envelopes above are sums of absolute values; the gradients are cancelling sums far below them.  So, as for dq / dk /
    # dv: d(logit_scale) per head against max(|ref|, rss / 4), rss = scale sqrt(sum (P (|dP| + P.|dP|) cosabs)^2) (independent errors
    # add in squares), and every scratch row on its own: d(logits) per (scratch row, head, query) and the d(logit_scale) partials
    live = ~ref.clamped
    res['dls_rel'] = _rel((dls - ref.dls).abs()[live], ref.dls.abs()[live], ref.rss_dls[live]) if live.any() else 0.0
    if scratch is not None:
        g, nw = ref.ds_g.shape[:2]
        scratch, part = scratch.double().cpu().view(g, nw, heads, n, n), part.double().cpu().view(g, nw, heads)
        assert (part[..., ref.clamped] == 0).all(), (tag, 'a clamped head has a logit-scale partial')
        res['scratch_rows'] = _rel((scratch - ref.ds_g).norm(dim=-1), ref.ds_g.norm(dim=-1), ref.m_ds_g.norm(dim=-1))
        res['dls_part_rel'] = _rel((part - ref.dls_g).abs()[..., live], ref.dls_g.abs()[..., live], ref.rss_dls_g[..., live]) \
            if live.any() else 0.0
    for k in ('dls_rel', 'scratch_rows', 'dls_part_rel'):
        if k in res:
            if record:
                record_distance(tag, k, row_rel_err=res[k])
            assert res[k] < frac * GRAD_GATE, (tag, k, res[k])
    return res
