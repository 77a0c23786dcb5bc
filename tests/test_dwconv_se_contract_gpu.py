"""The depthwise-convolution and squeeze-excite kernels (csrc/dwconv.hip, csrc/se.hip) across the whole contract of
include/tok.h, element by element against fp64: non-square and tiny maps, every tile width, grid-stride loops, odd batches,
row pitches with NaN input pads, sentinel output pads and guard rows, `+=` modes, nullable outputs and the argument refusals.

The bounds follow from where each kernel rounds (helpers.assert_bounded): bf16 results accumulated in fp32 get one bf16
rounding (2^-8 |ref|) plus 2^-16 of the magnitude term; fp32 results that are fixed-order sums of exact products get
2 d 2^-24 of the magnitude, d the longest chain of dependent additions, restated below from the .hip geometry."""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import Guarded, assert_bounded
from test_mnasnet_gpu import _se_ref
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
U32 = 2.0 ** -24                      # fp32 unit roundoff
A_BF, B_BF = 2.0 ** -8, 2.0 ** -16    # bf16 result accumulated in fp32
ERR_INVALID, ERR_WORKSPACE = -1, -3
KS = [(3, 1), (3, 2), (5, 1), (5, 2)]


# ---- the launch geometry of csrc/dwconv.hip, restated -------------------------------------------------------------------
GRID_CAP, STRIP = 2048, 4


def tile_groups(c):
    g = c >> 3
    for d in range(8, 1, -1):
        if g % d == 0:
            return d
    return 1


def dw_geo(out_rows, out_w, c, z):
    """dw_geo / grid_rows: channel groups per tile, pixel lanes, tiles, block rows, strips, strips a lane walks at most."""
    cg = tile_groups(c)
    lanes, tiles = 256 // cg, (c >> 3) // cg
    strips = out_rows * ((out_w + STRIP - 1) // STRIP)
    want = (strips + lanes - 1) // lanes
    rows = min(want, max(GRID_CAP // (tiles * z), 1))
    return dict(cg=cg, lanes=lanes, tiles=tiles, rows=rows, strips=strips, per_lane=-(-strips // (rows * lanes)))


def dw_chain(g):
    """longest chain of dependent fp32 additions of a wgrad / statistics sum: the strips of a lane (STRIP columns each), the
    lanes of a block folded in order, the block rows folded in order"""
    return g['per_lane'] * STRIP + g['lanes'] + g['rows']


def _odim(h, k, s):
    return (h + 2 * (k // 2) - k) // s + 1


def _check_rc(rc, msg, code=ERR_INVALID):
    err = _C.lib().tok_last_error()
    err = err.decode() if isinstance(err, bytes) else err
    assert rc == code, (rc, err)
    assert msg in err, (msg, err)


# ---- depthwise convolution ----------------------------------------------------------------------------------------------
def _dw_case(n, h, wd, c, k, s, ld, seed, tag):
    lib, st = _C.lib(), stream_ptr()
    g = torch.Generator().manual_seed(seed)
    p, q = _odim(h, k, s), _odim(wd, k, s)
    x = torch.randn(n, h, wd, c, generator=g).to(BF)
    w = torch.randn(c, k, k, generator=g) * (2.0 / (k * k)) ** 0.5
    dout = torch.randn(n, p, q, c, generator=g).to(BF)
    old_dx = torch.randn(n, h, wd, c, generator=g).to(BF)
    old_dw = torch.randn(c, k, k, generator=g)
    xg = Guarded(n * h * wd, c, ld, init=x, nan_pad=True)
    gg = Guarded(n * p * q, c, ld, init=dout, nan_pad=True)
    wc = w.cuda()

    # forward, with and without the statistics rows
    fwd = dw_geo(n * p, q, c, 1)
    rows = lib.tok_dwconv_rows(n, h, wd, c, k, s)
    assert rows == fwd['rows']
    out = Guarded(n * p * q, c, ld)
    out_ns = Guarded(n * p * q, c, ld)
    stats = Guarded(2 * rows, c, dtype=F32)
    _C.check(lib.tok_dwconv_fwd(xg.ptr, wc.data_ptr(), n, h, wd, c, ld, k, s, out.ptr, stats.ptr, st), 'fwd')
    _C.check(lib.tok_dwconv_fwd(xg.ptr, wc.data_ptr(), n, h, wd, c, ld, k, s, out_ns.ptr, None, st), 'fwd(no stats)')
    # data gradient (= and +=)
    dgr = dw_geo(n * h, wd, c, 1)
    dx = Guarded(n * h * wd, c, ld)
    dx_acc = Guarded(n * h * wd, c, ld, init=old_dx)
    _C.check(lib.tok_dwconv_dgrad(gg.ptr, wc.data_ptr(), n, h, wd, c, ld, k, s, dx.ptr, 0, st), 'dgrad')
    _C.check(lib.tok_dwconv_dgrad(gg.ptr, wc.data_ptr(), n, h, wd, c, ld, k, s, dx_acc.ptr, 1, st), 'dgrad(+=)')
    # weight gradient (= and +=)
    wgr = dw_geo(n * p, q, c, k)
    ws_bytes = lib.tok_dwconv_wgrad_ws_bytes(n, h, wd, c, k, s)
    assert ws_bytes == wgr['rows'] * c * k * k * 4
    ws = Guarded(wgr['rows'], c * k * k, dtype=F32)
    dw = Guarded(c, k * k, dtype=F32)
    dw_acc = Guarded(c, k * k, dtype=F32, init=old_dw)
    _C.check(lib.tok_dwconv_wgrad(xg.ptr, gg.ptr, n, h, wd, c, ld, k, s, dw.ptr, 0, ws.ptr, ws_bytes, st), 'wgrad')
    _C.check(lib.tok_dwconv_wgrad(xg.ptr, gg.ptr, n, h, wd, c, ld, k, s, dw_acc.ptr, 1, ws.ptr, ws_bytes, st), 'wgrad(+=)')
    torch.cuda.synchronize()
    for buf, what in ((out, 'out'), (out_ns, 'out(no stats)'), (stats, 'stats'), (dx, 'dx'), (dx_acc, 'dx(+=)'),
                      (ws, 'ws'), (dw, 'dw'), (dw_acc, 'dw(+=)')):
        buf.check(what)
    for buf, what in ((xg, 'x'), (gg, 'dout')):
        buf.check(what + ' (input)')

    # fp64 references and magnitude terms
    xd, gd = x.double().permute(0, 3, 1, 2), dout.double().permute(0, 3, 1, 2)
    wdd = w.double().view(c, 1, k, k)
    kw = dict(stride=s, padding=k // 2, groups=c)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(-1, c)           # noqa: E731
    ref = nhwc(F.conv2d(xd, wdd, **kw))
    mag = nhwc(F.conv2d(xd.abs(), wdd.abs(), **kw))
    ref_dx = nhwc(torch.nn.grad.conv2d_input(xd.shape, wdd, gd, **kw))
    mag_dx = nhwc(torch.nn.grad.conv2d_input(xd.shape, wdd.abs(), gd.abs(), **kw))
    ref_dw = torch.nn.grad.conv2d_weight(xd, wdd.shape, gd, **kw).view(c, k * k)
    mag_dw = torch.nn.grad.conv2d_weight(xd.abs(), wdd.shape, gd.abs(), **kw).view(c, k * k)

    o = out.value()
    assert torch.equal(o, out_ns.value()), 'forward output depends on whether statistics are requested'
    assert_bounded(o, ref, mag, A_BF, B_BF, 'dw fwd', tag)
    od = old_dx.double().reshape(-1, c)
    assert_bounded(dx.value(), ref_dx, mag_dx, A_BF, B_BF, 'dw dgrad', tag)
    assert_bounded(dx_acc.value(), od + ref_dx, od.abs() + mag_dx, A_BF, B_BF, 'dw dgrad +=', tag)
    d = dw_chain(wgr)
    assert_bounded(dw.value(), ref_dw, mag_dw, 0.0, 2 * d * U32, 'dw wgrad', tag)
    ow = old_dw.double().view(c, k * k)
    assert_bounded(dw_acc.value(), ow + ref_dw, ow.abs() + mag_dw, 0.0, 2 * (d + 1) * U32, 'dw wgrad +=', tag)
    # statistics of the ROUNDED output: every partial row written, folded in fp64 within the summation bound
    sv = stats.value().double().view(2, rows, c)
    assert torch.isfinite(sv).all()
    od64 = o.double()
    ds = dw_chain(fwd)
    assert_bounded(sv[0].sum(0), od64.sum(0), od64.abs().sum(0), 0.0, 2 * ds * U32, 'dw stats sum', tag)
    assert_bounded(sv[1].sum(0), (od64 * od64).sum(0), (od64 * od64).sum(0), 0.0, 2 * ds * U32, 'dw stats sumsq', tag)
    return fwd, dgr, wgr


SHAPES = [(9, 30), (30, 9), (1, 1), (1, 7), (2, 3), (5, 2), (13, 18)]


@pytest.mark.parametrize('h,wd', SHAPES)
@pytest.mark.parametrize('k,s', KS)
def test_dwconv_non_square_and_tiny_maps(k, s, h, wd):
    """odd batch, pitch c + 8; k = 5 on maps smaller than the filter, odd sizes at stride 2"""
    _dw_case(3, h, wd, 16, k, s, 16 + 8, seed=1000 * k + 100 * s + 10 * h + wd, tag=f'dw_contract/map{h}x{wd}_k{k}s{s}')


CHANNELS = [8, 16, 24, 32, 40, 48, 56, 88, 1152]


def test_dwconv_channel_list_covers_every_tile_width():
    assert {tile_groups(c) for c in CHANNELS} == set(range(1, 9))


@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('k,s', KS)
def test_dwconv_every_tile_width(k, s, c):
    """batch 1, pitch c + 24, a non-square map"""
    fwd, _, _ = _dw_case(1, 13, 18, c, k, s, c + 24, seed=c * 10 + k + s, tag=f'dw_contract/c{c}_k{k}s{s}')
    assert fwd['cg'] == tile_groups(c)


def test_dwconv_grid_stride_loops():
    """2048 channels (32 tiles of 8 groups): the 2048-workgroup cap binds and every lane of the forward, data-gradient and
    weight-gradient launches walks at least two strips"""
    n, h, wd, c, k, s = 1, 64, 256, 2048, 3, 1
    fwd, dgr, wgr = _dw_case(n, h, wd, c, k, s, c + 8, seed=7, tag='dw_contract/grid_stride')
    for what, g in (('fwd', fwd), ('dgrad', dgr), ('wgrad', wgr)):
        assert g['strips'] >= 2 * g['rows'] * g['lanes'], (what, g)


def test_dwconv_refusals():
    lib, st = _C.lib(), stream_ptr()
    n, h, wd = 1, 8, 8

    def bufs(c, ld, k, s):
        p, q = _odim(h, k, s), _odim(wd, k, s)
        x = torch.zeros(n * h * wd * ld, dtype=BF, device='cuda')
        o = torch.zeros(n * p * q * ld, dtype=BF, device='cuda')
        w = torch.zeros(c * k * k, dtype=F32, device='cuda')
        return x, o, w

    def run_all(c, ld, k, s, msg):
        x, o, w = bufs(c, ld, k, s)
        dw = torch.zeros(c * k * k, dtype=F32, device='cuda')
        ws = torch.zeros(max(c, 8) * k * k * 64, dtype=F32, device='cuda')
        _check_rc(lib.tok_dwconv_fwd(x.data_ptr(), w.data_ptr(), n, h, wd, c, ld, k, s, o.data_ptr(), None, st), msg)
        _check_rc(lib.tok_dwconv_dgrad(o.data_ptr(), w.data_ptr(), n, h, wd, c, ld, k, s, x.data_ptr(), 0, st), msg)
        _check_rc(lib.tok_dwconv_wgrad(x.data_ptr(), o.data_ptr(), n, h, wd, c, ld, k, s, dw.data_ptr(), 0, ws.data_ptr(),
                                       ws.numel() * 4, st), msg)
    run_all(16, 16, 7, 1, 'bad sizes')        # k = 7
    run_all(16, 16, 3, 3, 'bad sizes')        # stride 3
    run_all(12, 16, 3, 1, 'bad sizes')        # c % 8 != 0
    run_all(16, 8, 3, 1, 'bad sizes')         # ld < c
    run_all(16, 20, 3, 1, 'bad sizes')        # ld % 8 != 0
    for args in ((n, h, wd, 16, 7, 1), (n, h, wd, 16, 3, 3), (n, h, wd, 12, 3, 1)):
        assert lib.tok_dwconv_rows(*args) == ERR_INVALID
        assert lib.tok_dwconv_wgrad_ws_bytes(*args) == 0
    # workspace one float too small, null pointers
    c, k, s = 16, 3, 1
    x, o, w = bufs(c, c, k, s)
    dw = torch.zeros(c * k * k, dtype=F32, device='cuda')
    need = lib.tok_dwconv_wgrad_ws_bytes(n, h, wd, c, k, s)
    ws = torch.zeros(need // 4, dtype=F32, device='cuda')
    _check_rc(lib.tok_dwconv_wgrad(x.data_ptr(), o.data_ptr(), n, h, wd, c, c, k, s, dw.data_ptr(), 0, ws.data_ptr(), need - 4,
                                   st), 'workspace too small')
    P = (x.data_ptr(), w.data_ptr(), o.data_ptr())
    for i in range(3):
        a = list(P)
        a[i] = None
        _check_rc(lib.tok_dwconv_fwd(a[0], a[1], n, h, wd, c, c, k, s, a[2], None, st), 'null pointer')
        _check_rc(lib.tok_dwconv_dgrad(a[2], a[1], n, h, wd, c, c, k, s, a[0], 0, st), 'null pointer')
    P = (x.data_ptr(), o.data_ptr(), dw.data_ptr(), ws.data_ptr())
    for i in range(4):
        a = list(P)
        a[i] = None
        _check_rc(lib.tok_dwconv_wgrad(a[0], a[1], n, h, wd, c, c, k, s, a[2], 0, a[3], need, st), 'null pointer')
    torch.cuda.synchronize()
    assert not x.any() and not o.any() and not dw.any()        # nothing ran


# ---- squeeze-excite -----------------------------------------------------------------------------------------------------
SE_CAP = 2048


def se_geo(n, hw, c):
    """se_geo: channel groups per pass, pixel lanes per group, chunks per image (wanted / capped)"""
    cge = min(c >> 3, 256)
    rpb = 256 // cge
    want = -(-hw // (4 * rpb))
    cap = -(-SE_CAP // n)
    chunks = max(min(want, cap), 1)
    length = -(-hw // chunks)
    return dict(cge=cge, rpb=rpb, want=want, cap=cap, chunks=chunks, per_lane=-(-length // rpb))


def se_chain(g):
    """longest chain of the channel sums: the pixels of a lane, the lanes folded in order, the chunks folded in order"""
    return g['per_lane'] + g['rpb'] + g['chunks']


class _SE:
    """inputs of one squeeze-excite layer, its fp64 reference (autograd of _se_ref) and the magnitude terms"""

    def __init__(self, n, hw, c, rd, seed, dead=()):
        g = torch.Generator().manual_seed(seed)
        self.n, self.hw, self.c, self.rd = n, hw, c, rd
        self.x = torch.randn(n, hw, c, generator=g).abs().to(BF)
        self.w1, self.b1 = torch.randn(rd, c, generator=g) / c ** 0.5, torch.randn(rd, generator=g) * 0.1
        self.w2, self.b2 = torch.randn(c, rd, generator=g) / rd ** 0.5, torch.randn(c, generator=g) * 0.1
        for j in dead:
            self.b1[j] = -1e4                # dead hidden unit: relu(W1 mean + b1) == 0 in every image
        self.dout = torch.randn(n, hw, c, generator=g).to(BF)
        self._reference()

    def _reference(self):
        n, hw, c = self.n, self.hw, self.c
        prm = [t.double().requires_grad_() for t in (self.w1, self.b1, self.w2, self.b2)]
        xd = self.x.double().requires_grad_()
        gate = _se_ref(xd.view(n, hw, 1, c), *prm)
        (xd * gate[:, None, :] * self.dout.double()).sum().backward()
        with torch.no_grad():
            w1, b1, w2, b2 = (t.detach() for t in prm)
            x, dout = self.x.double(), self.dout.double()
            self.mean = x.mean(1)
            pre = self.mean @ w1.t() + b1
            self.hid = F.relu(pre)
            self.gate = gate.detach()
            self.dx = xd.grad
            self.grads = [t.grad for t in prm]                       # dW1, db1, dW2, db2
            # magnitude terms: the same chain on absolute values (the sigmoid / ReLU derivatives as the fixed factors they are)
            self.m_mean = x.abs().mean(1)
            self.m_hid = self.m_mean @ w1.abs().t() + b1.abs()
            self.m_gate = torch.sigmoid(self.m_hid @ w2.abs().t() + b2.abs())
            s = self.gate
            m_ds = (dout.abs() * x.abs()).sum(1) * s * (1 - s)
            m_dh = (pre > 0).double() * (m_ds @ w2.abs())
            self.m_grads = [m_dh.t() @ self.m_mean, m_dh.sum(0), m_ds.t() @ self.hid, m_ds.sum(0)]
            self.m_dx = dout.abs() * s[:, None, :] + (m_dh @ w1.abs())[:, None, :] / hw

    def device_params(self):
        return [t.cuda() for t in (self.w1, self.b1, self.w2, self.b2)]


def _se_fwd(se, ld, prm):
    lib = _C.lib()
    n, hw, c, rd = se.n, se.hw, se.c, se.rd
    xg = Guarded(n * hw, c, ld, init=se.x, nan_pad=True)
    mean, gate = Guarded(n, c, dtype=F32), Guarded(n, c, dtype=F32)
    hid = Guarded(n, rd, dtype=F32)
    ws = Guarded(1, lib.tok_se_ws_floats(n, hw, c, rd), dtype=F32)
    _C.check(lib.tok_se_fwd(xg.ptr, n, hw, c, ld, rd, *(t.data_ptr() for t in prm), mean.ptr, hid.ptr, gate.ptr, ws.ptr,
                            stream_ptr()), 'se_fwd')
    return xg, mean, hid, gate, ws


def _se_bwd(se, ld, prm, xg, mean, hid, gate, ws, grads, acc=0, dx=None, dx_acc=0, gg=None):
    """grads: four Guarded or None (null pointer)"""
    lib = _C.lib()
    n, hw, c, rd = se.n, se.hw, se.c, se.rd
    gg = gg or Guarded(n * hw, c, ld, init=se.dout, nan_pad=True)
    p = lambda t: None if t is None else t.ptr        # noqa: E731
    _C.check(lib.tok_se_bwd(gg.ptr, xg.ptr, n, hw, c, ld, rd, prm[0].data_ptr(), prm[2].data_ptr(), mean.ptr, hid.ptr,
                            gate.ptr, *(p(t) for t in grads), acc, p(dx), dx_acc, ws.ptr, stream_ptr()), 'se_bwd')
    return gg


GRAD_NAMES = ('dW1', 'db1', 'dW2', 'db2')


def _grad_bufs(se, init=None):
    shapes = ((se.rd, se.c), (1, se.rd), (se.c, se.rd), (1, se.c))
    return [Guarded(r, cc, dtype=F32, init=None if init is None else init[i]) for i, (r, cc) in enumerate(shapes)]


def _se_check(se, ld, tag, mean, hid, gate, grads, dx, prefill=None, old_dx=None):
    d = se_chain(se_geo(se.n, se.hw, se.c))
    assert_bounded(mean.value(), se.mean, se.m_mean, 0.0, 2 * d * U32, 'se mean', tag)
    assert_bounded(hid.value(), se.hid, se.m_hid, 0.0, 1e-3, 'se hid', tag)
    assert_bounded(gate.value(), se.gate, se.m_gate, 0.0, 1e-3, 'se gate', tag)
    for i, (buf, name) in enumerate(zip(grads, GRAD_NAMES)):
        ref, mag = se.grads[i].reshape(buf.rows, buf.cols), se.m_grads[i].reshape(buf.rows, buf.cols)
        if prefill is not None and prefill[i] is not None:
            old = prefill[i].double().reshape(ref.shape)
            ref, mag = old + ref, old.abs() + mag
        assert_bounded(buf.value(), ref, mag, 0.0, 1e-3, f'se {name}', tag)
    if dx is not None:
        ref, mag = se.dx.reshape(-1, se.c), se.m_dx.reshape(-1, se.c)
        if old_dx is not None:
            o = old_dx.double().reshape(ref.shape)
            ref, mag = o + ref, o.abs() + mag
        assert_bounded(dx.value(), ref, mag, A_BF, B_BF, 'se dx', tag)


def _se_full(n, hw, c, rd, ld, seed, tag, dead=()):
    se = _SE(n, hw, c, rd, seed, dead)
    prm = se.device_params()
    xg, mean, hid, gate, ws = _se_fwd(se, ld, prm)
    grads = _grad_bufs(se)
    dx = Guarded(n * hw, c, ld)
    gg = _se_bwd(se, ld, prm, xg, mean, hid, gate, ws, grads, 0, dx, 0)
    torch.cuda.synchronize()
    for b, what in zip([mean, hid, gate, ws, dx, xg, gg] + grads, ['mean', 'hid', 'gate', 'ws', 'dx', 'x', 'dout'] +
                       list(GRAD_NAMES)):
        b.check(what)
    _se_check(se, ld, tag, mean, hid, gate, grads, dx)
    return se, grads


@pytest.mark.parametrize('hw', [1, 49, 12544])
@pytest.mark.parametrize('c,rd', [(8, 1), (2048, 256), (2048, 1), (16, 256)])
def test_se_shapes(c, rd, hw):
    n = 1 if c * hw > 4_000_000 else 3
    _se_full(n, hw, c, rd, c + 8, seed=c + rd + hw, tag=f'se_contract/c{c}_rd{rd}_hw{hw}')


def test_se_chunk_cap_binds():
    n, hw, c = 64, 196, 2048
    g = se_geo(n, hw, c)
    assert g['want'] == 49 and g['cap'] == 32 and g['chunks'] == 32
    _se_full(n, hw, c, 64, c, seed=5, tag='se_contract/chunk_cap')


def test_se_dead_hidden_units():
    dead = (0, 3, 7)
    se, grads = _se_full(5, 49, 64, 8, 64 + 16, seed=9, tag='se_contract/dead', dead=dead)
    assert (se.hid[:, list(dead)] == 0).all()
    dw1, db1 = grads[0].value(), grads[1].value().view(-1)
    for j in dead:
        assert (db1[j] == 0).all() and (dw1[j] == 0).all(), j


def _se_setup(n=3, hw=49, c=48, rd=12, seed=17):
    se = _SE(n, hw, c, rd, seed)
    ld = c + 8
    prm = se.device_params()
    fwd = _se_fwd(se, ld, prm)
    return se, ld, prm, fwd


def test_se_param_accumulate_all_patterns():
    se, ld, prm, (xg, mean, hid, gate, ws) = _se_setup()
    fresh = _grad_bufs(se)
    _se_bwd(se, ld, prm, xg, mean, hid, gate, ws, fresh, 0)
    torch.cuda.synchronize()
    fresh_v = [b.value() for b in fresh]
    g = torch.Generator().manual_seed(3)
    for bits in range(16):
        pre = [torch.randn(b.rows, b.cols, generator=g) for b in fresh]
        bufs = _grad_bufs(se, pre)
        _se_bwd(se, ld, prm, xg, mean, hid, gate, ws, bufs, bits)
        torch.cuda.synchronize()
        for i, (b, name) in enumerate(zip(bufs, GRAD_NAMES)):
            b.check(name)
            want = pre[i] + fresh_v[i] if bits & (1 << i) else fresh_v[i]        # fp32 add, as the kernel does
            assert torch.equal(b.value(), want), (bits, name)
        _se_check(se, ld, f'se_contract/param_acc{bits}', mean, hid, gate, bufs, None,
                  prefill=[pre[i] if bits & (1 << i) else None for i in range(4)])


def test_se_null_gradients_and_dx():
    se, ld, prm, (xg, mean, hid, gate, ws) = _se_setup(seed=23)
    base = _grad_bufs(se)
    dx = Guarded(se.n * se.hw, se.c, ld)
    _se_bwd(se, ld, prm, xg, mean, hid, gate, ws, base, 0, dx, 0)
    torch.cuda.synchronize()
    base_v, dx_v = [b.value() for b in base], dx.value()
    for nulled in [(0,), (1,), (2,), (3,), (0, 1, 2, 3)]:
        bufs = _grad_bufs(se)                    # all sentinel: a nulled slot must stay so
        passed = [None if i in nulled else b for i, b in enumerate(bufs)]
        dx2 = Guarded(se.n * se.hw, se.c, ld)
        _se_bwd(se, ld, prm, xg, mean, hid, gate, ws, passed, 0, dx2, 0)
        torch.cuda.synchronize()
        for i, (b, name) in enumerate(zip(bufs, GRAD_NAMES)):
            if i in nulled:
                assert (b.buf.view(torch.int32) == b.bits).all(), (nulled, name)
            else:
                b.check(name)
                assert torch.equal(b.value(), base_v[i]), (nulled, name)
        dx2.check('dx')
        assert torch.equal(dx2.value(), dx_v), nulled
    # dx null: the parameter gradients unchanged; dx += onto a prefilled target
    bufs = _grad_bufs(se)
    _se_bwd(se, ld, prm, xg, mean, hid, gate, ws, bufs, 0, None, 0)
    old = torch.randn(se.n * se.hw, se.c, generator=torch.Generator().manual_seed(4)).to(BF)
    dx3 = Guarded(se.n * se.hw, se.c, ld, init=old)
    _se_bwd(se, ld, prm, xg, mean, hid, gate, ws, [None] * 4, 0, dx3, 1)
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        assert torch.equal(b.value(), base_v[i]), GRAD_NAMES[i]
    dx3.check('dx(+=)')
    _se_check(se, ld, 'se_contract/dx_acc', mean, hid, gate, base, dx3, old_dx=old)


def test_se_refusals():
    lib, st = _C.lib(), stream_ptr()
    n, hw = 2, 9
    for c, rd, ld in ((2056, 8, 2056), (16, 0, 16), (16, 257, 16), (16, 8, 8)):
        r1 = max(rd, 1)
        x = torch.zeros(n * hw * max(c, ld), dtype=BF, device='cuda')
        w1, w2 = torch.zeros(r1 * c, device='cuda'), torch.zeros(c * r1, device='cuda')
        b1, b2 = torch.zeros(r1, device='cuda'), torch.zeros(c, device='cuda')
        mean, gate = torch.zeros(n * c, device='cuda'), torch.zeros(n * c, device='cuda')
        hid = torch.zeros(n * r1, device='cuda')
        ws = torch.zeros(n * c * 64 + 2 * n * c + n * r1, device='cuda')
        grads = [torch.zeros_like(t) for t in (w1, b1, w2, b2)]
        dx = torch.zeros_like(x)
        P = lambda t: t.data_ptr()        # noqa: E731
        _check_rc(lib.tok_se_fwd(P(x), n, hw, c, ld, rd, P(w1), P(b1), P(w2), P(b2), P(mean), P(hid), P(gate), P(ws), st),
                  'bad sizes')
        _check_rc(lib.tok_se_bwd(P(x), P(x), n, hw, c, ld, rd, P(w1), P(w2), P(mean), P(hid), P(gate), *(P(t) for t in grads),
                                 0, P(dx), 0, P(ws), st), 'bad sizes')
        if ld == c:
            assert lib.tok_se_ws_floats(n, hw, c, rd) == 0
        torch.cuda.synchronize()
        assert not any(t.any() for t in [mean, hid, gate, dx] + grads)
