"""The references and bounds of tests/ocr_chan_ref.py, on a CPU:
  * every forward reference equals torch's own fp64 operation (torch.softmax, einsum / matmul, F.conv2d(groups=c)) and every
    backward reference fp64 autograd of that forward to 1e-12 relative, the accumulate forms and both `transposed` settings included;
  * the chains reproduce the oracle in fp64: softmax_cols_fwd -> weighted_pool is oracle.ocr_ref.spatial_gather, pix_class_matmul ->
    softmax_rows -> class_pix_expand the attention product of ObjectAttentionBlock, chan_gram(mode 1) -> chan_apply the core of
    oracle.davit_ref.ChannelAttention;
  * a plain fp32 run of every formula stays inside HALF of every bound on the inputs of every case of
    tests/test_ocr_chan_contract_gpu.py (and, rounded once to bf16 where the kernel stores bf16, inside the whole bound);
  * deliberately wrong variants do NOT pass;
  * the pad rule of tok_channel_scale (suspect 1 of the contract module) on the host stand-in tests/fake_backend.py."""
import pytest
import torch
import torch.nn.functional as F

from fake_backend import FakeTok
from helpers import BF, F32
import ocr_chan_ref as M
import oracle.davit_ref as OD
import oracle.ocr_ref as OO

F64 = torch.float64
TOL = dict(rtol=1e-12, atol=1e-13)
B = M.IMAGES


def half(what, mine32, out):
    """an fp32 run meets half of the fp32 part of the bound; rounded once to bf16 (where the kernel stores bf16) the whole bound"""
    w = M.check(None, what, mine32, out, frac=0.5, rounded=False)
    if bool((out.a > 0).any()):
        M.check(None, what + ' (bf16)', mine32.to(BF), out)
    return w


def rejected(what, wrong, out):
    with pytest.raises(AssertionError):
        M.check(None, what, wrong, out)


def grads(fn, inputs, dout):
    """fp64 autograd of fn at `inputs` against dout"""
    xs = [t.double().requires_grad_() for t in inputs]
    out = fn(*xs)
    out.backward(dout.double())
    return out.detach(), [x.grad for x in xs]


# ---- references against torch and autograd ------------------------------------------------------------------------------------------
def test_ocr_references_are_torch_and_autograd():
    d = M.make_ocr(B, 33, 19, 20, seed=1)
    x, m, w, pnc, pkc = d['x'], d['m'], d['w'], d['prior_nc'], d['prior_kc']
    torch.testing.assert_close(M.pix_class_matmul(x, m, 0.37), M.f32v(0.37) * torch.einsum('bnc,bkc->bnk', x.double(), m.double()), **TOL)
    torch.testing.assert_close(M.class_pix_expand(w, m, 0.37), M.f32v(0.37) * torch.einsum('bnk,bkc->bnc', w.double(), m.double()), **TOL)
    torch.testing.assert_close(M.class_pix_expand(w, m, 0.37, pnc), M.class_pix_expand(w, m, 0.37) + pnc.double(), **TOL)
    torch.testing.assert_close(M.weighted_pool(w, x, 0.25), M.f32v(0.25) * torch.einsum('bnk,bnc->bkc', w.double(), x.double()), **TOL)
    torch.testing.assert_close(M.weighted_pool(w, x, 0.25, pkc), M.weighted_pool(w, x, 0.25) + pkc.double(), **TOL)
    # the three products are each other's gradients: d<pcm(x, m), w> / dx = cpe(w, m), / dm = pool(w, x)
    _, (gx, gm) = grads(lambda a, b: M.f32v(0.37) * torch.einsum('bnc,bkc->bnk', a, b), (x, m), w)
    torch.testing.assert_close(M.class_pix_expand(w, m, 0.37), gx, **TOL)
    torch.testing.assert_close(M.weighted_pool(w, x, 0.37), gm, **TOL)

    xr, dpr = M.make_softmax_rows(37, 19, seed=2)
    p, (g,) = grads(lambda a: torch.softmax(a, -1), (xr,), dpr)
    torch.testing.assert_close(M.softmax_rows(xr), p, **TOL)
    torch.testing.assert_close(M.softmax_rows_bwd(p, dpr), g, **TOL)

    l, dp, prior = M.make_softmax_cols(B, 37, 19, seed=3)
    for scale in M.SC_SCALES:
        p, (g,) = grads(lambda a: torch.softmax(M.f32v(scale) * a, 1), (l,), dp)
        torch.testing.assert_close(M.softmax_cols_fwd(l, scale), p, **TOL)
        torch.testing.assert_close(M.softmax_cols_bwd(p, dp, scale), g, **TOL)
        torch.testing.assert_close(M.softmax_cols_bwd(p, dp, scale, prior), g + prior.double(), **TOL)

    xc, s, pr = M.make_channel_scale(B, 5, 20, seed=4)
    assert float(s[0, 0]) == 0 and float(s[B - 1, 19]) == float(torch.tensor(1 / 0.7, dtype=F32))
    torch.testing.assert_close(M.channel_scale(xc, s), xc.double() * s.double()[:, None, :], **TOL)
    torch.testing.assert_close(M.channel_scale(xc, s, pr), xc.double() * s.double()[:, None, :] + pr.double(), **TOL)


def _core(q, k, v, heads, scale):
    """ChannelAttention.forward between qkv and proj (oracle/davit_ref.py), on [b][n][c]"""
    b, n, c = q.shape
    q, k, v = (t.reshape(b, n, heads, c // heads).permute(0, 2, 1, 3) for t in (q, k, v))
    attn = ((k * scale).transpose(-1, -2) @ v).softmax(dim=-1)
    x = (attn @ q.transpose(-1, -2)).transpose(-1, -2)
    return x.transpose(1, 2).reshape(b, n, c), attn


def test_davit_references_are_torch_and_autograd():
    heads, rpi = 3, 65
    scale = M.f32v(32 ** -0.5)
    q, k, m, dout = M.make_chan(B, rpi, heads, seed=5)
    v = M.make_chan(B, rpi, heads, seed=6)[0]
    (out, attn), _ = _core(q.double(), k.double(), v.double(), heads, scale), None
    a = M.chan_gram(k, v, scale, 1)
    torch.testing.assert_close(a, attn.reshape(-1, 32, 32), **TOL)
    torch.testing.assert_close(M.chan_gram(k, v, scale, 0).softmax(-1), a, **TOL)
    torch.testing.assert_close(M.chan_apply(q, a, 0, 1.0), out, **TOL)
    # the backward of the engine (csrc/channel_attn.hip header): dS = mode 2 of dout^T q; dq = dout A; dk = scale v dS^T; dv = scale k dS
    _, (gq, gk, gv) = grads(lambda a_, b_, c_: _core(a_, b_, c_, heads, scale)[0], (q, k, v), dout)
    ds = M.chan_gram(dout, q, 1.0, 2, a)
    torch.testing.assert_close(M.chan_apply(dout, a, 1, 1.0), gq, **TOL)
    torch.testing.assert_close(M.chan_apply(v, ds, 0, scale), gk, **TOL)
    torch.testing.assert_close(M.chan_apply(k, ds, 1, scale), gv, **TOL)

    a_, b_, rs, prior = M.make_rows_add(50, 24, 16, seed=7)
    want = a_.double() + rs.double().repeat_interleave(16)[:50, None] * b_.double()
    torch.testing.assert_close(M.scale_rows_add(a_, b_, rs, 16), want, **TOL)
    torch.testing.assert_close(M.scale_rows_add(None, b_, rs, 16, prior), want - a_.double() + prior.double(), **TOL)
    torch.testing.assert_close(M.scale_rows_add(a_, b_, None, 0), a_.double() + b_.double(), **TOL)

    d = M.make_dwconv(B, 3, 5, 20, seed=8)
    x, wt, bias, g = d['x'], d['wt'], d['bias'], d['dout']

    def conv(xx, ww, bb):
        return F.conv2d(xx.permute(0, 3, 1, 2), ww.view(20, 1, 3, 3), bb, padding=1, groups=20).permute(0, 2, 3, 1)
    y, (gx, gw, gb) = grads(conv, (x, wt, bias), g)
    torch.testing.assert_close(M.dwconv3x3(x, wt, bias, 0), y, **TOL)
    torch.testing.assert_close(M.dwconv3x3(x, wt, None, 0, d['prior']), y - bias.double() + d['prior'].double(), **TOL)
    torch.testing.assert_close(M.dwconv3x3(g, wt, None, 1), gx, **TOL)
    dw, db = M.dwconv3x3_wgrad(x, g)
    torch.testing.assert_close(dw, gw, **TOL)
    torch.testing.assert_close(db, gb, **TOL)
    dw2, db2 = M.dwconv3x3_wgrad(x, g, d['prior_dw'], d['prior_db'])
    torch.testing.assert_close(dw2, gw + d['prior_dw'].double(), **TOL)
    torch.testing.assert_close(db2, gb + d['prior_db'].double(), **TOL)


# ---- chains against the oracle ---------------------------------------------------------------------------------------------------------
def test_chains_reproduce_the_oracle():
    b, k, c, h, w = B, 5, 12, 3, 4
    g = M.gen(9)
    feats, probs = torch.randn(b, c, h, w, generator=g, dtype=F64), torch.randn(b, k, h, w, generator=g, dtype=F64)
    x = feats.flatten(2).transpose(1, 2)             # [b][n][c]
    l = probs.flatten(2).transpose(1, 2)             # [b][n][k]
    for scale in (1, 0.5):
        ctx = M.weighted_pool(M.softmax_cols_fwd(l, scale), x, 1.0)            # [b][k][c]
        torch.testing.assert_close(ctx.transpose(1, 2).unsqueeze(3), OO.spatial_gather(feats, probs, scale), **TOL)
    # ObjectAttentionBlock: softmax(ck^-.5 q key) value
    ck = 8
    q, key, val = (torch.randn(s, generator=g, dtype=F64) for s in ((b, h * w, ck), (b, k, ck), (b, k, ck)))
    sc = M.f32v(ck ** -.5)                            # (the C ABI passes the scale as a float)
    want = torch.matmul(F.softmax(sc * torch.matmul(q, key.transpose(1, 2)), dim=-1), val)
    sim = M.softmax_rows(M.pix_class_matmul(q, key, sc).reshape(-1, k)).view(b, h * w, k)
    torch.testing.assert_close(M.class_pix_expand(sim, val, 1.0), want, **TOL)
    # ChannelAttention without its two Linear layers
    ca = OD.ChannelAttention(64, 2, True).double()
    ca.scale = M.f32v(ca.scale)
    xin = torch.randn(b, 10, 64, generator=g, dtype=F64)
    qkv = ca.qkv(xin)
    qq, kk, vv = qkv[..., :64], qkv[..., 64:128], qkv[..., 128:]
    core = M.chan_apply(qq, M.chan_gram(kk, vv, ca.scale, 1), 0, 1.0)
    torch.testing.assert_close(ca.proj(core), ca(xin), **TOL)


# ---- the fp32 run stays inside half of every bound ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,k,c,ldx,ldm,cls', M.PCM_CASES)
def test_pix_class_matmul_fp32(n, k, c, ldx, ldm, cls):
    assert M.pcm_class(n, c) == cls
    d = M.make_ocr(B, n, k, c, seed=n + k + c)
    for scale in (1.0, 0.37):
        half('out', M.pix_class_matmul(d['x'], d['m'], scale, F32), M.pix_class_matmul_ref(d['x'], d['m'], scale))


@pytest.mark.parametrize('n,k,c,ldm,ldo,cls', M.CPE_CASES)
def test_class_pix_expand_fp32(n, k, c, ldm, ldo, cls):
    assert M.grid_class(n * M.cdiv(c, 8), 1024) == cls
    d = M.make_ocr(B, n, k, c, seed=n + k + c)
    for scale in (1.0, 0.37):
        for prior in (None, d['prior_nc']):
            half('out', M.class_pix_expand(d['w'], d['m'], scale, prior, F32), M.class_pix_expand_ref(d['w'], d['m'], scale, prior))


@pytest.mark.parametrize('case,cls', list(zip(M.WP_CASES, M.WP_CLASSES)))
def test_weighted_pool_fp32(case, cls):
    n, k, c, ldx, ldo = case
    assert M.pool_class(n, k, c) == cls
    d = M.make_ocr(B, n, k, c, seed=n + k + c)
    for prior in (None, d['prior_kc']):
        out = M.weighted_pool_ref(d['w'], d['x'], 0.25, prior)
        half('out', M.weighted_pool(d['w'], d['x'], 0.25, prior, F32), out)
        if k > 1 and prior is None:
            assert bool((out.ref[:, k - 1] == 0).all()) and bool((out.bound()[:, k - 1] == 0).all()), 'a class of zero weights pools to exactly 0'


@pytest.mark.parametrize('rows,k', M.SR_CASES)
def test_softmax_rows_fp32(rows, k):
    x, dp = M.make_softmax_rows(rows, k, seed=rows + k)
    p32 = M.softmax_rows(x, F32)
    half('p', p32, M.softmax_rows_ref(x))
    half('dx', M.softmax_rows_bwd(p32, dp, F32), M.softmax_rows_bwd_ref(p32, dp))


@pytest.mark.parametrize('n,k,ld', M.SC_CASES)
def test_softmax_cols_fp32(n, k, ld):
    l, dp, prior = M.make_softmax_cols(B, n, k, seed=n + k)
    for scale in M.SC_SCALES:
        p32 = M.softmax_cols_fwd(l, scale, F32)
        half('p', p32, M.softmax_cols_fwd_ref(l, scale))
        for pr in (None, prior):
            half('dlogits', M.softmax_cols_bwd(p32, dp, scale, pr, F32), M.softmax_cols_bwd_ref(p32, dp, scale, pr))


@pytest.mark.parametrize('n,c,ld,cls', M.CS_CASES)
def test_channel_scale_fp32(n, c, ld, cls):
    assert M.grid_class(n * (ld // 8), 1024) == cls
    x, s, prior = M.make_channel_scale(B, n, c, seed=n + c)
    for pr in (None, prior):
        half('out', M.channel_scale(x, s, pr, F32), M.channel_scale_ref(x, s, pr))


@pytest.mark.parametrize('heads', M.HEADS)
@pytest.mark.parametrize('rpi', M.CG_RPI)
def test_chan_gram_fp32(rpi, heads):
    scale = 32 ** -0.5
    x, y, _, dout = M.make_chan(B, rpi, heads, seed=rpi + heads)
    g = M.chan_gram(x, y, scale, 0)
    assert float(g[0, 0, 0]) > 50, 'the planted logit'
    half('G', M.chan_gram(x, y, scale, 0, None, F32), M.chan_gram_ref(x, y, scale, 0))
    a32 = M.chan_gram(x, y, scale, 1, None, F32)
    half('A', a32, M.chan_gram_ref(x, y, scale, 1))
    half('dS', M.chan_gram(dout, x, 1.0, 2, a32, F32), M.chan_gram_ref(dout, x, 1.0, 2, a32))


@pytest.mark.parametrize('heads', M.HEADS)
@pytest.mark.parametrize('rpi', M.CA_RPI)
def test_chan_apply_fp32(rpi, heads):
    x, _, m, _ = M.make_chan(B, rpi, heads, seed=rpi + heads)
    for transposed in (0, 1):
        for scale in (1.0, 32 ** -0.5):
            half('out', M.chan_apply(x, m, transposed, scale, F32), M.chan_apply_ref(x, m, transposed, scale))


@pytest.mark.parametrize('rows,ld,rps,with_a,acc', M.SRA_CASES)
def test_scale_rows_add_fp32(rows, ld, rps, with_a, acc):
    a, b, rs, prior = M.make_rows_add(rows, ld, rps, seed=rows + ld)
    a, prior = (a if with_a else None), (prior if acc else None)
    half('out', M.scale_rows_add(a, b, rs, rps, prior, F32), M.scale_rows_add_ref(a, b, rs, rps, prior))


@pytest.mark.parametrize('c', [c for c, _ in M.DW_COLS])
@pytest.mark.parametrize('h,w', M.DW_MAPS)
def test_dwconv3x3_fp32(h, w, c):
    d = M.make_dwconv(B, h, w, c, seed=h + w + c)
    for bias in (None, d['bias']):
        for flip in (0, 1):
            for prior in (None, d['prior']):
                half('out', M.dwconv3x3(d['x'], d['wt'], bias, flip, prior, F32), M.dwconv3x3_ref(d['x'], d['wt'], bias, flip, prior))


def test_dwconv3x3_second_trip_case_fp32():
    n, h, w, c, _ = M.DW_BIG
    d = M.make_dwconv(n, h, w, c, seed=11)
    half('out', M.dwconv3x3(d['x'], d['wt'], d['bias'], 0, None, F32), M.dwconv3x3_ref(d['x'], d['wt'], d['bias'], 0))


@pytest.mark.parametrize('n,h,w,c,ld,geo', M.DWG_CASES)
def test_dwconv3x3_wgrad_fp32(n, h, w, c, ld, geo):
    assert M.wgrad_geometry(n, h) == geo
    d = M.make_dwconv(n, h, w, c, seed=n + h)
    for pw, pb in ((None, None), (d['prior_dw'], d['prior_db'])):
        ref = M.dwconv3x3_wgrad_ref(d['x'], d['dout'], pw, pb)
        dw, db = M.dwconv3x3_wgrad(d['x'], d['dout'], pw, pb, F32)
        half('dw', dw, ref['dw'])
        half('db', db, ref['db'])


# ---- wrong variants --------------------------------------------------------------------------------------------------------------------
def test_wrong_variants_are_rejected():
    l, dp, prior = M.make_softmax_cols(B, 37, 19, seed=3)
    lf = l.float()
    rejected('softmax over the classes instead of the pixels', torch.softmax(0.37 * lf, 2), M.softmax_cols_fwd_ref(l, 0.37))
    rejected('scale dropped from softmax_cols_fwd', torch.softmax(lf, 1), M.softmax_cols_fwd_ref(l, 0.37))
    p32 = M.softmax_cols_fwd(l, 0.37, F32)
    rejected('scale dropped from softmax_cols_bwd', M.softmax_cols_bwd(p32, dp, 1.0, None, F32), M.softmax_cols_bwd_ref(p32, dp, 0.37))
    rejected('softmax_cols_bwd that overwrites under accumulate', M.softmax_cols_bwd(p32, dp, 0.37, None, F32), M.softmax_cols_bwd_ref(p32, dp, 0.37, prior))
    rejected('softmax_cols_bwd over the classes', p32 * (dp - (p32 * dp).sum(2, keepdim=True)) * 0.37, M.softmax_cols_bwd_ref(p32, dp, 0.37))
    xr, dpr = M.make_softmax_rows(37, 19, seed=2)
    rejected('softmax_rows over the rows', torch.softmax(xr, 0), M.softmax_rows_ref(xr))
    pr32 = M.softmax_rows(xr, F32)
    rejected('softmax_rows_bwd without the dot', pr32 * dpr, M.softmax_rows_bwd_ref(pr32, dpr))

    x, y, m, dout = M.make_chan(B, 65, 3, seed=5)
    for tr in (0, 1):
        rejected('transposed flipped', M.chan_apply(x, m, 1 - tr, 0.5, F32), M.chan_apply_ref(x, m, tr, 0.5))
    a32 = M.chan_gram(x, y, 32 ** -0.5, 1, None, F32)
    g32 = M.chan_gram(dout, x, 1.0, 0, None, F32)
    rejected('rowsum dropped in mode 2', a32 * g32, M.chan_gram_ref(dout, x, 1.0, 2, a32))
    rejected('mode 1 over the columns', torch.softmax(M.chan_gram(x, y, 32 ** -0.5, 0, None, F32), 1), M.chan_gram_ref(x, y, 32 ** -0.5, 1))
    rejected('mode 1 through a bf16 rounding', a32.to(BF), M.chan_gram_ref(x, y, 32 ** -0.5, 1))

    a, b, rs, _ = M.make_rows_add(50, 24, 16, seed=7)
    wrong = a.float() + rs[torch.arange(50) % 16 % len(rs)][:, None] * b.float()
    rejected('row / rps replaced by row % rps', wrong, M.scale_rows_add_ref(a, b, rs, 16))

    d = M.make_dwconv(B, 3, 5, 20, seed=8)
    rejected('flip ignored', M.dwconv3x3(d['dout'], d['wt'], None, 0, None, F32), M.dwconv3x3_ref(d['dout'], d['wt'], None, 1))
    rejected('bias dropped', M.dwconv3x3(d['x'], d['wt'], None, 0, None, F32), M.dwconv3x3_ref(d['x'], d['wt'], d['bias'], 0))
    # an output stored through one extra bf16 rounding: the convolution rounded to bf16 BEFORE the prior is added
    rejected('an extra bf16 rounding before the add of the prior',
             M.dwconv3x3(d['x'], d['wt'], d['bias'], 0, None, F32).to(BF).float() + d['prior'].float(), M.dwconv3x3_ref(d['x'], d['wt'], d['bias'], 0, d['prior']))
    ref = M.dwconv3x3_wgrad_ref(d['x'], d['dout'])
    dw32, db32 = M.dwconv3x3_wgrad(d['x'], d['dout'], None, None, F32)
    rejected('dw with the taps reversed', dw32.flip(1), ref['dw'])
    rejected('db of x instead of dout', d['x'].float().sum((0, 1, 2)), ref['db'])

    o = M.make_ocr(B, 33, 19, 20, seed=1)
    rejected('pix_class_matmul without scale', M.pix_class_matmul(o['x'], o['m'], 1.0, F32), M.pix_class_matmul_ref(o['x'], o['m'], 0.37))
    rejected('class_pix_expand through bf16 weights', M.class_pix_expand(o['w'].to(BF), o['m'], 1.0, None, F32), M.class_pix_expand_ref(o['w'], o['m'], 1.0))
    rejected('class_pix_expand rounded to bf16 before the add of the prior',
             M.class_pix_expand(o['w'], o['m'], 1.0, None, F32).to(BF).float() + o['prior_nc'].float(), M.class_pix_expand_ref(o['w'], o['m'], 1.0, o['prior_nc']))
    rejected('weighted_pool of the other image', M.weighted_pool(o['w'].flip(0), o['x'], 1.0, None, F32), M.weighted_pool_ref(o['w'], o['x'], 1.0))
    xc, s, pr = M.make_channel_scale(B, 5, 20, seed=4)
    rejected('channel_scale with the gate of the other image', M.channel_scale(xc, s.flip(0), None, F32), M.channel_scale_ref(xc, s))
    rejected('channel_scale that overwrites under accumulate', M.channel_scale(xc, s, None, F32), M.channel_scale_ref(xc, s, pr))


# ---- suspect 1 on the host stand-in -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('acc', [0, 1])
def test_channel_scale_stand_in_keeps_pads_out_of_results(acc):
    """tok_channel_scale computed x * 0 on the pad columns c..ld, so a NaN in a pad of x became a NaN in the pad of out.  The rule of
    include/tok.h now: the pad columns of x are not read into a result; out's are written 0 when fresh and keep what they held under
    accumulate.  The stand-in mirrors it."""
    images, n, c, ld = 2, 3, 20, 24
    x, s, prior = M.make_channel_scale(images, n, c, seed=1)
    xb = torch.full((images, n, ld), float('nan'), dtype=BF)
    xb[..., :c] = x
    ob = torch.full((images, n, ld), 7.0, dtype=BF)
    ob[..., :c] = prior
    sc = s.contiguous()
    assert FakeTok().tok_channel_scale(xb.data_ptr(), sc.data_ptr(), ob.data_ptr(), acc, images, n, c, ld, None) == 0
    assert bool((ob[..., c:] == (7.0 if acc else 0.0)).all())
    M.check(None, 'out', ob[..., :c], M.channel_scale_ref(x, s, prior if acc else None))
