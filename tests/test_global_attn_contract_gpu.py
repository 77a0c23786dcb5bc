"""The global-attention kernels (csrc/attn_global.hip) across the contract of include/tok.h: token counts up to
TOK_GLOBAL_ATTN_MAX_TOKENS, many (image, head) pairs, NaN input pads with sentinel output pads and guard rows, sharp and
constant logits, a zero output gradient and the argument refusals.

Forward: element by element |out - ref| <= 2^-8 |ref| + 2^-7 (P @ |V|) (P is rounded to bf16 before the PV MFMA while the row
sum stays fp32: about 2^-8 of P @ |V|, doubled for margin).  Backward: the worst per-token-row relative error of dq, dk and dv,
each row measured against max(|ref row|, |magnitude row| / 4) (one bf16 rounding of the result plus one of P or dS on the
magnitude: 2^-8 (1 + 4) < 2e-2), gated at the whole-tensor 2e-2 of test_vit_gpu.py."""
import pytest
import torch

from helpers import Guarded, assert_bounded, record_distance
from test_vit_gpu import _attn
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
HD = 64


def _launch(qkv, b, n, heads, dout, ldq, ldo, ldd):
    """forward + backward on guarded buffers (NaN input pads, sentinel output pads and guard rows)"""
    lib, st = _C.lib(), stream_ptr()
    c = heads * HD
    qg = Guarded(b * n, 3 * c, ldq, init=qkv, nan_pad=True)
    og = Guarded(b * n, c, ldo)
    lg = Guarded(b * heads, n, dtype=F32)
    _C.check(lib.tok_global_attn_fwd(qg.ptr, ldq, b, n, heads, HD, og.ptr, ldo, lg.ptr, st), 'fwd')
    gg = Guarded(b * n, c, ldo, init=dout, nan_pad=True)
    dg = Guarded(b * n, 3 * c, ldd)
    ws_bytes = lib.tok_global_attn_bwd_ws_bytes(b, n, heads)
    wsg = Guarded(1, ws_bytes // 4, dtype=F32)
    _C.check(lib.tok_global_attn_bwd(qg.ptr, ldq, og.ptr, gg.ptr, ldo, lg.ptr, b, n, heads, HD, dg.ptr, ldd, wsg.ptr, ws_bytes,
                                     st), 'bwd')
    torch.cuda.synchronize()
    for buf, what in ((qg, 'qkv'), (og, 'out'), (lg, 'lse'), (gg, 'dout'), (dg, 'dqkv'), (wsg, 'ws')):
        buf.check(what)
    return og.value(), lg.value(), dg.value()


class _Ref:
    """fp64 forward / backward of the same bf16 inputs and the magnitude terms of every result"""

    def __init__(self, qkv, b, n, heads, dout):
        c = heads * HD
        x = qkv.double().requires_grad_(True)
        q, k, v = x.reshape(b, n, 3, heads, HD).permute(2, 0, 3, 1, 4)
        s = (q @ k.transpose(-2, -1)) * 0.125
        p = s.softmax(-1)
        o = p @ v
        o.transpose(1, 2).reshape(b * n, c).backward(dout.double())
        with torch.no_grad():
            go = dout.double().reshape(b, n, heads, HD).transpose(1, 2)
            self.out = o.detach().transpose(1, 2).reshape(b * n, c)
            self.lse = torch.logsumexp(s.detach(), -1)
            pd, qa, ka, va, ga = p.detach(), q.detach().abs(), k.detach().abs(), v.detach().abs(), go.abs()
            self.m_out = (pd @ va).transpose(1, 2).reshape(b * n, c)
            m_ds = pd * (ga @ va.transpose(-2, -1) + (ga * o.detach().abs()).sum(-1, keepdim=True))
            tok = lambda t: t.transpose(1, 2).reshape(b * n, c)        # noqa: E731
            self.m_grad = [tok(0.125 * m_ds @ ka), tok(0.125 * m_ds.transpose(-2, -1) @ qa), tok(pd.transpose(-2, -1) @ ga)]
            self.grad = [x.grad[:, i * c:(i + 1) * c] for i in range(3)]


def _check(tag, ref, out, lse, dqkv, heads, gate=2e-2):
    c = heads * HD
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv.float()).all()
    assert (out.double() - ref.out).norm() / ref.out.norm().clamp_min(1e-300) < 1e-2       # the whole-tensor gate, kept
    assert_bounded(out, ref.out, ref.m_out, 2.0 ** -8, 2.0 ** -7, 'attn out', tag)
    lse_err = float((lse.double().view(ref.lse.shape) - ref.lse).abs().max())
    assert lse_err < 1e-3, lse_err
    for i, what in enumerate(('dq', 'dk', 'dv')):
        mine, want, mag = dqkv[:, i * c:(i + 1) * c].double(), ref.grad[i], ref.m_grad[i]
        # (plus 2^-24 of the largest magnitude row: a row of ~e^-120-weighted terms underflows to 0 in fp32)
        den = torch.maximum(torch.maximum(want.norm(dim=1), mag.norm(dim=1) / 4), mag.norm(dim=1).max() * 2.0 ** -24)
        e = (mine - want).norm(dim=1)
        worst = float(torch.where(den > 0, e / den.clamp_min(1e-300), torch.where(e > 0, float('inf'), 0.0)).max())
        record_distance(tag, what, row_rel_err=worst)
        assert worst < gate, (what, worst)


def _inputs(b, n, heads, seed, scale=1.5):
    c = heads * HD
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(b * n, 3 * c, generator=g) * scale).to(BF)
    dout = torch.randn(b * n, c, generator=g).to(BF)
    return qkv, dout


def _case(b, n, heads, qkv, dout, tag):
    c = heads * HD
    out, lse, dqkv = _launch(qkv.cuda(), b, n, heads, dout.cuda(), 3 * c + 8, c + 24, 3 * c + 16)
    ref = _Ref(qkv, b, n, heads, dout)
    _check(tag, ref, out, lse, dqkv, heads)
    return ref, out, lse, dqkv


@pytest.mark.parametrize('n,heads', [(2048, 1), (2305, 2), (4095, 1), (4096, 2)])
def test_long_token_counts(n, heads):
    qkv, dout = _inputs(1, n, heads, seed=n + heads)
    _case(1, n, heads, qkv, dout, f'attn_contract/n{n}_h{heads}')


def test_many_image_head_pairs():
    b, n, heads = 4, 197, 12
    qkv, dout = _inputs(b, n, heads, seed=197)
    _case(b, n, heads, qkv, dout, 'attn_contract/b4_h12')


def test_sharp_logits():
    """rows nearly one-hot: head 0 puts every query's maximum on the last key (in the last, partial key tile: the running
    maximum moves ~128 nats at the end), head 1 on key 0 (every later tile lies ~120 nats below the running maximum)"""
    b, n, heads = 1, 200, 2
    c = heads * HD
    g = torch.Generator().manual_seed(31)
    qkv = torch.randn(n, 3 * c, generator=g) * 0.5
    for h, key in ((0, n - 1), (1, 0)):
        e = torch.where(torch.rand(HD, generator=g) < 0.5, -0.125, 0.125)
        qkv[:, h * HD:(h + 1) * HD] += 32 * e                          # queries
        qkv[:, c + h * HD:c + (h + 1) * HD] *= 0.1                     # small keys ...
        qkv[key, c + h * HD:c + (h + 1) * HD] = 32 * e                 # ... but one, aligned with every query
    qkv = qkv.to(BF)
    dout = torch.randn(n, c, generator=g).to(BF)
    ref, *_ = _case(b, n, heads, qkv, dout, 'attn_contract/sharp')
    q, k = qkv.double().reshape(n, 3, heads, HD)[:, 0], qkv.double().reshape(n, 3, heads, HD)[:, 1]
    s = torch.einsum('ihd,jhd->hij', q, k) * 0.125
    assert (s.softmax(-1).amax(-1) > 0.999).all()
    assert (s.argmax(-1)[0] == n - 1).all() and (s.argmax(-1)[1] == 0).all()


def test_constant_logits():
    """q = 0: uniform rows, the output is the mean of V over the n keys (n not a multiple of 64)"""
    b, n, heads = 2, 100, 1
    c = heads * HD
    qkv, dout = _inputs(b, n, heads, seed=8)
    qkv[:, :c] = 0
    _, out, lse, _ = _case(b, n, heads, qkv, dout, 'attn_contract/constant')
    v = qkv[:, 2 * c:].double().view(b, n, c)
    mean_v = v.mean(1, keepdim=True).expand(b, n, c).reshape(b * n, c)
    assert_bounded(out, mean_v, v.abs().mean(1, keepdim=True).expand(b, n, c).reshape(b * n, c), 2.0 ** -8, 2.0 ** -7,
                   'attn out = mean V', 'attn_contract/constant')
    ln_n = torch.log(torch.tensor(float(n), dtype=torch.float64))
    assert (lse.double() - ln_n).abs().max() < 4e-6        # a few fp32 ulps of ln(100)


def test_zero_output_gradient():
    b, n, heads = 2, 130, 3
    qkv, _ = _inputs(b, n, heads, seed=12)
    dout = torch.zeros(b * n, heads * HD, dtype=BF)
    _, _, dqkv = _launch(qkv.cuda(), b, n, heads, dout.cuda(), 3 * heads * HD, heads * HD + 8, 3 * heads * HD + 8)
    assert (dqkv == 0).all()
    ldo = heads * HD
    _, _, dq2 = _attn(qkv.cuda(), b, n, heads, ldo, dout.cuda())       # the launcher of test_vit_gpu.py: same answer
    assert (dq2.cpu()[:, :3 * heads * HD] == 0).all()


def _check_rc(rc, code, msg):
    err = _C.lib().tok_last_error()
    err = err.decode() if isinstance(err, bytes) else err
    assert rc == code, (rc, err)
    assert msg in err, (msg, err)


def test_refusals():
    lib, st = _C.lib(), stream_ptr()

    def bufs(b, n, heads, ldd_cols=None):
        c = heads * HD
        qkv = torch.zeros(b * n, 3 * c, dtype=BF, device='cuda')
        out = torch.zeros(b * n, c, dtype=BF, device='cuda')
        lse = torch.zeros(b * heads * n, dtype=F32, device='cuda')
        dqkv = torch.zeros(b * n, ldd_cols or 3 * c, dtype=BF, device='cuda')
        ws = torch.zeros(max(lib.tok_global_attn_bwd_ws_bytes(b, n, heads), 256) // 4, dtype=F32, device='cuda')
        return qkv, out, lse, dqkv, ws

    def fwd(b, n, heads, t):
        c = heads * HD
        return lib.tok_global_attn_fwd(t[0].data_ptr(), 3 * c, b, n, heads, HD, t[1].data_ptr(), c, t[2].data_ptr(), st)

    def bwd(b, n, heads, t, ldd=None, ws_bytes=None):
        c = heads * HD
        return lib.tok_global_attn_bwd(t[0].data_ptr(), 3 * c, t[1].data_ptr(), t[1].data_ptr(), c, t[2].data_ptr(), b, n, heads,
                                       HD, t[3].data_ptr(), ldd or 3 * c, t[4].data_ptr(),
                                       t[4].numel() * 4 if ws_bytes is None else ws_bytes, st)
    # 4097 tokens
    t = bufs(1, 4097, 1)
    _check_rc(fwd(1, 4097, 1, t), -1, 'tokens')
    _check_rc(bwd(1, 4097, 1, t), -1, 'tokens')
    # batch * heads = 65536
    t = bufs(256, 1, 256)
    _check_rc(fwd(256, 1, 256, t), -1, 'batch * heads')
    _check_rc(bwd(256, 1, 256, t), -1, 'batch * heads')
    # ldd < 3C, workspace one byte short
    b, n, heads = 2, 70, 2
    t = bufs(b, n, heads)
    _check_rc(bwd(b, n, heads, t, ldd=3 * heads * HD - 8), -1, 'ldd')
    need = lib.tok_global_attn_bwd_ws_bytes(b, n, heads)
    _check_rc(bwd(b, n, heads, t, ws_bytes=need - 1), -3, 'workspace')
    torch.cuda.synchronize()
    assert not t[3].any() and not t[1].any()
