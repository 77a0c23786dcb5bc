"""The grouped 3x3 convolution kernels (csrc/conv_group.hip) across the contract of include/tok.h, element by element against
fp64 (tests/gconv_ref.py): every served group width, both strides, a ragged 16-channel tile, tiny and odd maps, grid-stride
loops, row pitches with NaN input pads, sentinel output pads and guard rows, both weight layouts, `+=` modes, the nullable
statistics and the argument refusals.

Two kinds of data.  Small integers: every product and every sum is exact in the formats the kernels use, so out, dx, dw and the
statistics must equal the fp64 reference bit for bit — an index or group-boundary error cannot hide inside a tolerance.  Reals:
bf16 results accumulated in fp32 get one bf16 rounding (2^-8 |ref|) plus 2^-16 of the magnitude term; fp32 results that are
fixed-order sums of exact products get 2 d 2^-24 of the magnitude, d the longest chain of dependent additions restated in
gconv_ref from the .hip geometry."""
import pytest
import torch

import gconv_ref as G
from helpers import Guarded, assert_bounded
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
U32 = 2.0 ** -24                      # fp32 unit roundoff
A_BF, B_BF = 2.0 ** -8, 2.0 ** -16    # bf16 result accumulated in fp32
ERR_INVALID = -1

MAP_A, MAP_B, MAP_C, MAP_D, MAP_E, MAP_F = (3, 1, 1), (2, 2, 3), (3, 7, 5), (2, 9, 9), (2, 57, 33), (1, 56, 56)
# (groups, cg, stride, (n, h, w), pitch - c)
CASES = [
    (6, 4, 1, MAP_A, 0), (6, 4, 1, MAP_C, 8), (6, 4, 1, MAP_E, 0), (6, 4, 2, MAP_B, 0), (6, 4, 2, MAP_C, 0), (6, 4, 2, MAP_D, 8),
    (2, 4, 1, MAP_B, 8), (2, 4, 1, MAP_D, 0), (2, 4, 2, MAP_C, 0), (2, 4, 2, MAP_A, 0),
    (3, 8, 1, MAP_C, 0), (3, 8, 1, MAP_E, 8), (3, 8, 2, MAP_D, 0), (3, 8, 2, MAP_B, 0),
    (3, 16, 1, MAP_D, 16), (3, 16, 1, MAP_A, 0), (3, 16, 2, MAP_C, 8), (3, 16, 2, MAP_E, 0),
    (2, 32, 1, MAP_C, 0), (2, 32, 1, MAP_B, 0), (2, 32, 2, MAP_D, 8), (2, 32, 2, MAP_E, 0),
    (2, 64, 1, MAP_D, 0), (2, 64, 1, MAP_C, 8), (2, 64, 2, MAP_C, 0), (2, 64, 2, MAP_B, 0),
    (64, 4, 1, MAP_E, 0), (64, 4, 1, MAP_B, 0), (64, 4, 2, MAP_E, 8), (64, 4, 2, MAP_C, 0),
    (32, 4, 1, MAP_F, 0), (32, 4, 2, MAP_F, 0),          # the first grouped layer of resnext50_32x4d
    (8, 64, 1, MAP_E, 0), (8, 64, 2, MAP_E, 0),          # 512 channels: the workgroup caps bind, see test_grid_stride_...
]
IDS = [f'g{g}x{cg}_s{s}_{n}x{h}x{w}_pad{e}' for g, cg, s, (n, h, w), e in CASES]


def test_case_list_covers_the_contract():
    assert {cg for _, cg, _, _, _ in CASES} == set(G.WIDTHS)
    for cg in G.WIDTHS:
        assert {s for _, c2, s, _, _ in CASES if c2 == cg} == {1, 2}, cg
    assert any(s == 2 and h % 2 == 1 and w % 2 == 1 for _, _, s, (_, h, w), _ in CASES)
    assert any(e > 0 for *_, e in CASES) and any(e == 0 for *_, e in CASES)
    assert any((g * cg) % 16 == 8 for g, cg, *_ in CASES)          # a ragged 16-channel tile


def test_grid_stride_loops_take_more_than_one_trip():
    """at 512 channels on the 57 x 33 map a wave of each launch walks more than one tile / chunk"""
    n, h, w = MAP_E
    assert G.geo(n * h * w, 512, 8)['trips'] > 1
    assert G.wgrad_geo(n * h * w, 512, 8)['trips'] > 1
    assert G.wgrad_geo(n * G.odim(h, 2) * G.odim(w, 2), 512, 8)['trips'] > 1


def _check_rc(rc, msg, code=ERR_INVALID):
    err = _C.lib().tok_last_error()
    err = err.decode() if isinstance(err, bytes) else err
    assert rc == code, (rc, err)
    assert msg in err, (msg, err)


def _data(kind, n, h, wd, p, q, c, cg, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 'int':
        ri = lambda *s: torch.randint(-2, 3, s, generator=g).float()          # noqa: E731
        x, dout, old_dx = ri(n, h, wd, c).to(BF), ri(n, p, q, c).to(BF), ri(n, h, wd, c).to(BF)
        w = torch.randint(-1, 2, (c, cg, 3, 3), generator=g).float()
        if cg >= 32:                                     # thinner filters keep the widest sums inside bf16's integers
            w = w * (torch.rand(c, cg, 3, 3, generator=g) < 0.5)
        old_dw = ri(c, cg, 3, 3)
    else:
        x = torch.randn(n, h, wd, c, generator=g).to(BF)
        dout = torch.randn(n, p, q, c, generator=g).to(BF)
        old_dx = torch.randn(n, h, wd, c, generator=g).to(BF)
        w = torch.randn(c, cg, 3, 3, generator=g) * (2.0 / (9 * cg)) ** 0.5
        old_dw = torch.randn(c, cg, 3, 3, generator=g)
    return x, w, dout, old_dx, old_dw


def _assert_exactly_representable(ref, old_dx, old_dw):
    """The integer check is only as good as the exactness of every sum, so that is asserted on the reference first: every fp32
    sum (any partial sum is bounded by the sum of magnitudes) stays below 2^24 and every bf16 result within bf16's integers."""
    c = ref.out.shape[1]
    od = old_dx.double().reshape(-1, c)
    for mag in (ref.out_mag, ref.dx_mag + od.abs(), ref.dw_mag + old_dw.double().abs(), ref.out_mag.sum(0),
                (ref.out * ref.out).sum(0)):
        assert float(mag.max()) < 2 ** 24
    for res in (ref.out, ref.dx, od + ref.dx):
        assert float(res.abs().max()) <= 2 ** 8


def _layout(t, krsc):
    """the (c, cg, 3, 3) tensor as the flat memory image of the layout `krsc` names, and back"""
    return (t.permute(0, 2, 3, 1) if krsc else t).contiguous().reshape(-1)


def _unlayout(flat, c, cg, krsc):
    return flat.view(c, 3, 3, cg).permute(0, 3, 1, 2) if krsc else flat.view(c, cg, 3, 3)


def _run(kind, groups, cg, s, nhw, extra, krsc, seed, tag):
    lib, st = _C.lib(), stream_ptr()
    n, h, wd = nhw
    c, ld = groups * cg, groups * cg + extra
    p, q = G.odim(h, s), G.odim(wd, s)
    x, w, dout, old_dx, old_dw = _data(kind, n, h, wd, p, q, c, cg, seed)
    ref = G.Ref(x, w, dout, groups, s)
    exact = kind == 'int'
    if exact:
        _assert_exactly_representable(ref, old_dx, old_dw)

    xg = Guarded(n * h * wd, c, ld, init=x, nan_pad=True)
    gg = Guarded(n * p * q, c, ld, init=dout, nan_pad=True)
    wc = _layout(w, krsc).cuda()
    wc0 = wc.clone()

    fwd, dgr, wgr = G.geo(n * p * q, c, groups), G.geo(n * h * wd, c, groups), G.wgrad_geo(n * p * q, c, groups)
    rows = lib.tok_gconv_rows(n, h, wd, c, groups, s)
    assert rows == fwd['rows']
    ws_bytes = lib.tok_gconv_wgrad_ws_bytes(n, h, wd, c, groups, s)
    assert ws_bytes == wgr['ws_bytes']

    def forward(xbuf, with_stats=True):
        out = Guarded(n * p * q, c, ld)
        stats = Guarded(2 * rows, c, dtype=F32) if with_stats else None
        _C.check(lib.tok_gconv_fwd(xbuf.ptr, wc.data_ptr(), krsc, n, h, wd, c, ld, groups, s, out.ptr,
                                   stats.ptr if with_stats else None, st), 'fwd')
        return out, stats

    def dgrad(gbuf, init=None):
        dx = Guarded(n * h * wd, c, ld, init=init)
        _C.check(lib.tok_gconv_dgrad(gbuf.ptr, wc.data_ptr(), krsc, n, h, wd, c, ld, groups, s, dx.ptr, int(init is not None), st),
                 'dgrad')
        return dx

    def wgrad(init=None):
        ws = Guarded(1, ws_bytes // 4, dtype=F32)
        dw = Guarded(1, c * cg * 9, dtype=F32, init=None if init is None else _layout(init, krsc))
        _C.check(lib.tok_gconv_wgrad(xg.ptr, gg.ptr, n, h, wd, c, ld, groups, s, dw.ptr, krsc, int(init is not None), ws.ptr,
                                     ws_bytes, st), 'wgrad')
        return dw, ws

    out, stats = forward(xg)
    out_ns, _ = forward(xg, with_stats=False)
    out2, stats2 = forward(xg)
    dx, dx_acc, dx2 = dgrad(gg), dgrad(gg, init=old_dx), dgrad(gg)
    (dw, ws), (dw_acc, ws_a), (dw2, ws2) = wgrad(), wgrad(init=old_dw), wgrad()
    # group isolation: other values in the input channels of ONE group leave every other group's results alone
    gsel = groups // 2
    lo, hi = gsel * cg, (gsel + 1) * cg
    x_alt, g_alt = x.clone(), dout.clone()
    x_alt[..., lo:hi] = (x_alt[..., lo:hi].float() * -2 + 1).to(BF)
    g_alt[..., lo:hi] = (g_alt[..., lo:hi].float() * -2 + 1).to(BF)
    out_alt, _ = forward(Guarded(n * h * wd, c, ld, init=x_alt, nan_pad=True))
    dx_alt = dgrad(Guarded(n * p * q, c, ld, init=g_alt, nan_pad=True))
    torch.cuda.synchronize()

    for buf, what in ((out, 'out'), (out_ns, 'out(no stats)'), (stats, 'stats'), (dx, 'dx'), (dx_acc, 'dx(+=)'), (ws, 'ws'),
                      (dw, 'dw'), (dw_acc, 'dw(+=)'), (ws_a, 'ws(+=)'), (out_alt, 'out(alt)'), (dx_alt, 'dx(alt)')):
        buf.check(what)
    for buf, what in ((xg, 'x'), (gg, 'dout')):
        buf.check(what + ' (input)')
    assert torch.equal(xg.value(), x.view(-1, c)) and torch.equal(gg.value(), dout.view(-1, c)), 'an input was written'
    assert torch.equal(wc, wc0), 'the weight was written'

    o = out.value()
    assert torch.equal(o, out_ns.value()), 'forward output depends on whether statistics are requested'
    # run to run, bit for bit
    assert torch.equal(o, out2.value()) and torch.equal(stats.value(), stats2.value())
    assert torch.equal(dx.value(), dx2.value()) and torch.equal(dw.value(), dw2.value())
    # group isolation
    keep = torch.ones(c, dtype=torch.bool)
    keep[lo:hi] = False
    assert torch.equal(o[:, keep], out_alt.value()[:, keep]), 'a group reads another group\'s input channels'
    assert not torch.equal(o[:, ~keep], out_alt.value()[:, ~keep])
    assert torch.equal(dx.value()[:, keep], dx_alt.value()[:, keep]), 'a group\'s dx reads another group\'s dout channels'
    assert not torch.equal(dx.value()[:, ~keep], dx_alt.value()[:, ~keep])

    od = old_dx.double().reshape(-1, c)
    ow = old_dw.double()
    dwv = _unlayout(dw.value().view(-1), c, cg, krsc)
    dwa = _unlayout(dw_acc.value().view(-1), c, cg, krsc)
    sv = stats.value().double().view(2, rows, c)
    assert torch.isfinite(sv).all()
    s_sum, s_sq, s_abs = G.stats_ref(o)
    if exact:
        assert torch.equal(o.double(), ref.out), 'forward'
        assert torch.equal(dx.value().double(), ref.dx), 'dgrad'
        assert torch.equal(dx_acc.value().double(), od + ref.dx), 'dgrad +='
        assert torch.equal(dwv.double(), ref.dw), 'wgrad'
        assert torch.equal(dwa.double(), ow + ref.dw), 'wgrad +='
        assert torch.equal(sv[0].sum(0), s_sum) and torch.equal(sv[1].sum(0), s_sq), 'statistics'
        return
    assert_bounded(o, ref.out, ref.out_mag, A_BF, B_BF, 'gconv fwd', tag)
    assert_bounded(dx.value(), ref.dx, ref.dx_mag, A_BF, B_BF, 'gconv dgrad', tag)
    assert_bounded(dx_acc.value(), od + ref.dx, od.abs() + ref.dx_mag, A_BF, B_BF, 'gconv dgrad +=', tag)
    d = G.wgrad_chain(wgr)
    assert_bounded(dwv, ref.dw, ref.dw_mag, 0.0, 2 * d * U32, 'gconv wgrad', tag)
    assert_bounded(dwa, ow + ref.dw, ow.abs() + ref.dw_mag, 0.0, 2 * (d + 1) * U32, 'gconv wgrad +=', tag)
    ds = G.stats_chain(fwd)
    assert_bounded(sv[0].sum(0), s_sum, s_abs, 0.0, 2 * ds * U32, 'gconv stats sum', tag)
    assert_bounded(sv[1].sum(0), s_sq, s_sq, 0.0, 2 * ds * U32, 'gconv stats sumsq', tag)


@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_gconv_integers_bit_for_bit(i):
    g, cg, s, nhw, extra = CASES[i]
    _run('int', g, cg, s, nhw, extra, krsc=i % 2, seed=100 + i, tag=None)


@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_gconv_reals_within_format_bounds(i):
    g, cg, s, nhw, extra = CASES[i]
    _run('real', g, cg, s, nhw, extra, krsc=(i + 1) % 2, seed=500 + i, tag=f'gconv_contract/{IDS[i]}')


def test_gconv_refusals():
    lib, st = _C.lib(), stream_ptr()
    n, h, wd = 1, 8, 8
    served = '{4, 8, 16, 32, 64}'

    def run_all(c, ld, groups, s, msg=served):
        big = max(c, ld, 8)
        x = torch.zeros(n * h * wd * big, dtype=BF, device='cuda')
        o = torch.zeros(n * h * wd * big, dtype=BF, device='cuda')
        w = torch.zeros(big * 64 * 9, dtype=F32, device='cuda')
        dw = torch.zeros(big * 64 * 9, dtype=F32, device='cuda')
        ws = torch.zeros(1 << 20, dtype=F32, device='cuda')
        for krsc in (0, 1):
            _check_rc(lib.tok_gconv_fwd(x.data_ptr(), w.data_ptr(), krsc, n, h, wd, c, ld, groups, s, o.data_ptr(), None, st), msg)
            _check_rc(lib.tok_gconv_dgrad(o.data_ptr(), w.data_ptr(), krsc, n, h, wd, c, ld, groups, s, x.data_ptr(), 0, st), msg)
            _check_rc(lib.tok_gconv_wgrad(x.data_ptr(), o.data_ptr(), n, h, wd, c, ld, groups, s, dw.data_ptr(), krsc, 0,
                                          ws.data_ptr(), ws.numel() * 4, st), msg)
        torch.cuda.synchronize()
        assert not x.any() and not o.any() and not dw.any() and not ws.any()        # nothing ran
    run_all(24, 24, 2, 1)          # cg = 12
    run_all(256, 256, 2, 1)        # cg = 128
    run_all(16, 16, 8, 1)          # cg = 2
    run_all(24, 24, 5, 1)          # c % groups != 0
    run_all(16, 16, 1, 1)          # groups == 1: the dense route
    run_all(12, 16, 3, 1)          # c % 8 != 0
    run_all(16, 8, 2, 1)           # ld < c
    run_all(16, 20, 2, 1)          # ld % 8 != 0
    run_all(16, 16, 2, 3)          # stride 3
    for args in ((n, h, wd, 24, 2, 1), (n, h, wd, 24, 5, 1), (n, h, wd, 16, 1, 1), (n, h, wd, 12, 3, 1), (n, h, wd, 16, 2, 3)):
        assert lib.tok_gconv_rows(*args) == ERR_INVALID
        assert lib.tok_gconv_wgrad_ws_bytes(*args) == 0
    # workspace one float too small, null pointers
    c, groups, s = 16, 2, 1
    x = torch.zeros(n * h * wd * c, dtype=BF, device='cuda')
    o = torch.zeros(n * h * wd * c, dtype=BF, device='cuda')
    w = torch.zeros(c * 8 * 9, dtype=F32, device='cuda')
    dw = torch.zeros(c * 8 * 9, dtype=F32, device='cuda')
    need = lib.tok_gconv_wgrad_ws_bytes(n, h, wd, c, groups, s)
    assert need > 0
    ws = torch.zeros(need // 4, dtype=F32, device='cuda')
    _check_rc(lib.tok_gconv_wgrad(x.data_ptr(), o.data_ptr(), n, h, wd, c, c, groups, s, dw.data_ptr(), 0, 0, ws.data_ptr(),
                                  need - 4, st), 'workspace too small')
    P = (x.data_ptr(), w.data_ptr(), o.data_ptr())
    for i in range(3):
        a = list(P)
        a[i] = None
        _check_rc(lib.tok_gconv_fwd(a[0], a[1], 0, n, h, wd, c, c, groups, s, a[2], None, st), 'null pointer')
        _check_rc(lib.tok_gconv_dgrad(a[2], a[1], 0, n, h, wd, c, c, groups, s, a[0], 0, st), 'null pointer')
    P = (x.data_ptr(), o.data_ptr(), dw.data_ptr(), ws.data_ptr())
    for i in range(4):
        a = list(P)
        a[i] = None
        _check_rc(lib.tok_gconv_wgrad(a[0], a[1], n, h, wd, c, c, groups, s, a[2], 0, 0, a[3], need, st), 'null pointer')
    torch.cuda.synchronize()
    assert not x.any() and not o.any() and not dw.any()        # nothing ran
