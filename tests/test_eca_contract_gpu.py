"""The ECA residual kernels (csrc/eca.hip: tok_eca_fwd / tok_eca_bwd) across the contract of include/tok.h, element by element
against fp64 (tests/eca_ref.py): the smallest shape, a padded pitch with NaN input pads, sentinel output pads and guard rows, a
7x7 map, several chunks per image, the channel cap, a window wider than half the channels, `=` and `+=` for each output, each
output NULL in turn, run-to-run bits, the bit-for-bit cases (exact inputs, the mask read from the stored output, locality of the
window, independence of the images) and the argument refusals.

Each stage is held to its own inputs: `mean` and `gate` against fp64 of z and w; `out` against fp64 of z, the shortcut and the
gate the library stored; the backward against fp64 of its arguments (dout, the stored out, z, w and the stored mean and gate are
what tok_eca_bwd is given).  Bounds (helpers.assert_bounded): a bf16 result accumulated in fp32 gets one bf16 rounding
(2^-8 |ref|) plus 2^-16 of the magnitude term; an fp32 fixed-order sum gets 2 d 2^-24 of the magnitude, d the longest chain of
dependent additions, restated below from the .hip geometry; the gate lies within 1e-3 of its magnitude term (the figure
tests/test_dwconv_se_contract_gpu.py uses for the same sigmoid_f)."""
import pytest
import torch
import torch.nn.functional as F

import eca_ref as E
from helpers import Guarded, assert_bounded
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
U32 = 2.0 ** -24                      # fp32 unit roundoff
A_BF, B_BF = 2.0 ** -8, 2.0 ** -16    # bf16 result accumulated in fp32
ERR_INVALID = -1
GRID_CAP, TAP_ROW = 2048, 16

# (n, hw, c, k, ld)
SHAPES = [(1, 1, 8, 3, 8), (3, 5, 24, 5, 32), (2, 49, 64, 3, 64), (2, 1200, 64, 9, 64), (1, 16, 2048, 7, 2048), (2, 16, 8, 7, 8)]


# ---- the launch geometry of csrc/eca.hip, restated ---------------------------------------------------------------------------
def eca_geo(n, hw, c):
    """eca_geo / chunk_rows: channel groups across the block, row lanes, chunks per image, pixels per chunk"""
    cge = min(c // 8, 256)
    rpb = 256 // cge
    want = -(-hw // (4 * rpb))
    chunks = max(1, min(want, -(-GRID_CAP // n)))
    return dict(cge=cge, rpb=rpb, chunks=chunks, len=-(-hw // chunks))


def pixel_chain(g):
    """longest chain of dependent fp32 additions of a per-(image, channel) sum over the pixels: the rows of a lane, the row lanes
    of a block folded in order (those that had a row: adding the exact zero of an idle lane rounds nothing), the chunks folded in
    order"""
    return -(-g['len'] // g['rpb']) + (min(g['rpb'], g['len']) - 1) + g['chunks']


def dw_chain(g, n, c, k):
    """dw[j]: the roundings of da (the pixel chain, then two products), a lane's channels in order, the six steps of the wave's
    butterfly, the images in order"""
    return pixel_chain(g) + 3 + -(-c // 64) + 6 + n


def ws_floats(n, hw, c):
    return n * eca_geo(n, hw, c)['chunks'] * c + n * c + n * TAP_ROW


def _window(v, w):
    k = w.numel()
    return F.conv1d(v.unsqueeze(1), w.view(1, 1, k), padding=k // 2).squeeze(1)


class Case:
    """inputs of one shape (bf16 values kept in fp32 tensors on the host) and what the library made of them"""

    def __init__(self, n, hw, c, k, ld, seed=0, ints=False, zero_w=False):
        self.n, self.hw, self.c, self.k, self.ld = n, hw, c, k, ld
        g = torch.Generator().manual_seed(seed)
        if ints:       # small integers: every product and sum below is exact in fp32
            self.z = (torch.randint(-4, 5, (n, hw, c), generator=g) * 2).float()
            self.sc = torch.randint(-4, 5, (n, hw, c), generator=g).float()
            self.dout = torch.randint(-3, 4, (n, hw, c), generator=g).float()
        else:
            self.z = torch.randn(n, hw, c, generator=g).to(BF).float()
            self.sc = torch.randn(n, hw, c, generator=g).to(BF).float()
            self.dout = torch.randn(n, hw, c, generator=g).to(BF).float()
        self.w = torch.zeros(k) if zero_w else torch.randn(k, generator=g) * 0.7
        self.old_dz = torch.randn(n, hw, c, generator=g).to(BF).float()
        self.old_ds = torch.randn(n, hw, c, generator=g).to(BF).float()
        self.old_dw = torch.randn(k, generator=g)

    def rows(self, t, nan_pad=True):
        return Guarded(self.n * self.hw, self.c, self.ld, init=t.to(BF), nan_pad=nan_pad)

    def forward(self):
        lib, n, hw, c, k, ld = _C.lib(), self.n, self.hw, self.c, self.k, self.ld
        assert lib.tok_eca_ws_floats(n, hw, c) == ws_floats(n, hw, c)
        self.zg, self.sg = self.rows(self.z), self.rows(self.sc)
        self.wd = self.w.cuda()
        self.mean, self.gate = Guarded(n, c, dtype=F32), Guarded(n, c, dtype=F32)
        self.out = Guarded(n * hw, c, ld)
        self.ws = Guarded(1, ws_floats(n, hw, c), dtype=F32)
        _C.check(lib.tok_eca_fwd(self.zg.ptr, self.sg.ptr, n, hw, c, ld, self.wd.data_ptr(), k, self.mean.ptr, self.gate.ptr,
                                 self.out.ptr, self.ws.ptr, stream_ptr()), 'tok_eca_fwd')
        torch.cuda.synchronize()
        for b, what in ((self.mean, 'mean'), (self.gate, 'gate'), (self.out, 'out'), (self.ws, 'ws'), (self.zg, 'z (input)'),
                        (self.sg, 'shortcut (input)')):
            b.check(what)
        return self

    def backward(self, dw='new', dz='new', ds='new', acc=(0, 0, 0)):
        """each of dw / dz / ds: 'new' (a sentinel buffer), 'old' (prefilled), None (a NULL pointer) -> the three buffers"""
        lib, n, hw, c, k, ld = _C.lib(), self.n, self.hw, self.c, self.k, self.ld
        self.gg = self.rows(self.dout)
        mk = lambda how, make: None if how is None else make(how == 'old')      # noqa: E731
        bw = mk(dw, lambda old: Guarded(1, k, dtype=F32, init=self.old_dw if old else None))
        bz = mk(dz, lambda old: Guarded(n * hw, c, ld, init=self.old_dz.to(BF) if old else None))
        bs = mk(ds, lambda old: Guarded(n * hw, c, ld, init=self.old_ds.to(BF) if old else None))
        p = lambda t: None if t is None else t.ptr        # noqa: E731
        _C.check(lib.tok_eca_bwd(self.gg.ptr, self.out.ptr, self.zg.ptr, n, hw, c, ld, self.wd.data_ptr(), k, self.mean.ptr,
                                 self.gate.ptr, p(bw), acc[0], p(bz), acc[1], p(bs), acc[2], self.ws.ptr, stream_ptr()),
                 'tok_eca_bwd')
        torch.cuda.synchronize()
        for b, what in ((bw, 'dw'), (bz, 'dz'), (bs, 'dshort'), (self.ws, 'ws'), (self.gg, 'dout (input)'), (self.out, 'out'),
                        (self.mean, 'mean'), (self.gate, 'gate')):
            if b is not None:
                b.check(what)
        return bw, bz, bs

    # ---- fp64 ------------------------------------------------------------------------------------------------------------------
    def check_forward(self, tag):
        n, hw, c = self.n, self.hw, self.c
        d = pixel_chain(eca_geo(n, hw, c))
        _, mean, gate = E.eca_residual_ref(self.z, self.sc, self.w)
        m_mean = self.z.double().abs().mean(1)
        assert_bounded(self.mean.value(), mean, m_mean, 0.0, 2 * (d + 1) * U32, 'mean', tag)
        assert_bounded(self.gate.value(), gate, torch.sigmoid(_window(m_mean, self.w.double().abs())), 0.0, 1e-3, 'gate', tag)
        g = self.gate.value().double().unsqueeze(1)            # the gate pass 2 was given
        z, sc = self.z.double(), self.sc.double()
        assert_bounded(self.out.value().view(n, hw, c), torch.relu(z * g + sc), z.abs() * g + sc.abs(), A_BF, B_BF, 'out', tag)

    def backward_ref(self):
        out = self.out.value().double().view(self.n, self.hw, self.c)
        mean, gate = self.mean.value().double(), self.gate.value().double()
        r = E.eca_residual_bwd_ref(self.dout, out, self.z, self.w, mean, gate)
        k, c, wabs = self.k, self.c, self.w.double().abs()
        m_da = (r['dshort'].abs() * self.z.double().abs()).sum(1) * gate * (1 - gate)
        mp = F.pad(mean.abs(), (k // 2, k // 2))
        r['m_dw'] = torch.stack([(m_da * mp[:, j:j + c]).sum() for j in range(k)])
        r['m_dz'] = r['dshort'].abs() * gate.unsqueeze(1) + _window(m_da, wabs.flip(0)).unsqueeze(1) / self.hw
        return r

    def check_backward(self, tag, bw, bz, bs, acc=(0, 0, 0)):
        n, hw, c, k = self.n, self.hw, self.c, self.k
        g = eca_geo(n, hw, c)
        r = self.backward_ref()
        # the fp32 part of a bf16 result stays below 2^-16 of its magnitude: the chain into dmean is short enough
        assert 2 * pixel_chain(g) + k + 6 <= 256
        if bw is not None:
            old = self.old_dw.double() if acc[0] else torch.zeros(k, dtype=torch.float64)
            assert_bounded(bw.value().view(k), r['dw'] + old, r['m_dw'] + old.abs(), 0.0,
                           2 * (dw_chain(g, n, c, k) + 1) * U32, 'dw' + '(+=)' * acc[0], tag)
        if bz is not None:
            old = self.old_dz.double() if acc[1] else torch.zeros_like(r['dz'])
            assert_bounded(bz.value().view(n, hw, c), r['dz'] + old, r['m_dz'] + old.abs(), A_BF, B_BF, 'dz' + '(+=)' * acc[1], tag)
        if bs is not None:
            old = self.old_ds.double() if acc[2] else torch.zeros_like(r['dz'])
            assert_bounded(bs.value().view(n, hw, c), r['dshort'] + old, r['dshort'].abs() + old.abs(), A_BF, B_BF,
                           'dshort' + '(+=)' * acc[2], tag)
        return r


# ---- every shape, = and += ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,hw,c,k,ld', SHAPES)
def test_shapes_against_fp64(n, hw, c, k, ld):
    tag = f'eca_contract/{n}x{hw}x{c}k{k}'
    if (n, hw, c) == (2, 1200, 64):
        assert eca_geo(n, hw, c)['chunks'] == 10           # more than one chunk per image
    if (n, hw, c) == (3, 5, 24):
        assert ld > c
    case = Case(n, hw, c, k, ld, seed=n * 100 + k).forward()
    case.check_forward(tag)
    case.check_backward(tag, *case.backward())
    acc = (1, 1, 1)
    case.check_backward(tag + '/acc', *case.backward('old', 'old', 'old', acc), acc=acc)


def test_accumulate_flags_one_at_a_time():
    case = Case(3, 5, 24, 5, 32, seed=11).forward()
    base = [b.value() for b in case.backward()]
    for i in range(3):
        acc = tuple(int(j == i) for j in range(3))
        bufs = case.backward(*('old' if a else 'new' for a in acc), acc=acc)
        case.check_backward(f'eca_contract/acc{i}', *bufs, acc=acc)
        for j, b in enumerate(bufs):
            if j != i:
                assert torch.equal(b.value(), base[j]), (i, j)          # the other two: what `=` gives
        if i == 0:
            assert torch.equal(bufs[0].value().view(-1), case.old_dw + base[0].view(-1))      # one fp32 add, as the kernel does


def test_null_outputs_and_identical_calls():
    case = Case(2, 49, 64, 3, 64, seed=12).forward()
    base = [b.value() for b in case.backward()]
    again = [b.value() for b in case.backward()]
    for a, b in zip(base, again):
        assert torch.equal(a, b)                                        # two identical calls, identical bits
    for i in range(3):
        how = ['new'] * 3
        how[i] = None
        bufs = case.backward(*how)
        assert bufs[i] is None
        for j, b in enumerate(bufs):
            if j != i:
                assert torch.equal(b.value(), base[j]), (i, j)
    # dshort alone needs neither the sums nor the per-image math: the workspace is not touched
    case.ws.view.copy_(torch.full_like(case.ws.view, 7.0))
    bufs = case.backward(None, None, 'new')
    assert torch.equal(bufs[2].value(), base[2]) and bool((case.ws.value() == 7.0).all())
    # the forward twice
    other = Case(2, 49, 64, 3, 64, seed=12).forward()
    for a, b in ((case.mean, other.mean), (case.gate, other.gate), (case.out, other.out)):
        assert torch.equal(a.value(), b.value())


# ---- bit for bit ------------------------------------------------------------------------------------------------------------
def test_exact_inputs_round_once():
    """small integers, hw a power of two, w = 0: the gate is exactly 0.5, dmean is 0 and every sum is exact in fp32, so out, dz,
    dshort and dw are the fp64 results rounded once; the mask is the stored out > 0, also where z g + shortcut is exactly 0"""
    n, hw, c, k = 3, 4, 24, 5
    case = Case(n, hw, c, k, 32, seed=13, ints=True, zero_w=True).forward()
    assert bool((case.gate.value() == 0.5).all())
    assert torch.equal(case.mean.value().double(), case.z.double().mean(1))
    pre = case.z.double() * 0.5 + case.sc.double()
    want_out = torch.relu(pre).to(BF)
    assert torch.equal(case.out.value().view(n, hw, c), want_out)
    bw, bz, bs = case.backward()
    r = case.backward_ref()
    zero_pre = (pre == 0) & (case.dout != 0)
    assert int(zero_pre.sum()) > 0 and int((pre < 0).sum()) > 0 and int((pre > 0).sum()) > 0
    dm = case.dout.double() * (pre > 0)
    assert torch.equal(r['dshort'], dm)
    assert torch.equal(bs.value().view(n, hw, c).double(), dm)
    assert torch.equal(bz.value().view(n, hw, c), (dm * 0.5).to(BF))
    assert bool((bz.value().view(n, hw, c)[zero_pre] == 0).all()) and bool((bs.value().view(n, hw, c)[zero_pre] == 0).all())
    assert bool((r['dmean'] == 0).all()) and bool((r['dw'] != 0).any())
    assert torch.equal(bw.value().view(k), r['dw'].float()) and torch.equal(bw.value().view(k).double(), r['dw'])


def test_window_is_local():
    """another value in channel j of z (image 0) leaves `out` of that image bit-identical outside channels j +- k // 2, and moves
    the gates inside"""
    n, hw, c, k, j = 2, 16, 64, 9, 30
    a = Case(n, hw, c, k, 64, seed=14).forward()
    b = Case(n, hw, c, k, 64, seed=14)
    b.z[0, :, j] += 1.0
    b.z = b.z.to(BF).float()
    b.forward()
    oa, ob = a.out.value().view(n, hw, c), b.out.value().view(n, hw, c)
    inside = torch.zeros(c, dtype=torch.bool)
    inside[j - k // 2:j + k // 2 + 1] = True
    assert torch.equal(oa[0][:, ~inside], ob[0][:, ~inside]) and torch.equal(oa[1], ob[1])
    ga, gb = a.gate.value(), b.gate.value()
    assert torch.equal(ga[0][~inside], gb[0][~inside]) and bool((ga[0][inside] != gb[0][inside]).all())


def test_images_are_independent():
    n, hw, c, k = 2, 16, 64, 5
    a = Case(n, hw, c, k, 64, seed=15).forward()
    b = Case(n, hw, c, k, 64, seed=15)
    g = torch.Generator().manual_seed(16)
    for t in (b.z, b.sc, b.dout):
        t[1] = torch.randn(hw, c, generator=g).to(BF).float()
    b.forward()
    ra, rb = a.backward(), b.backward()
    for x, y, what in ((a.mean, b.mean, 'mean'), (a.gate, b.gate, 'gate')):
        assert torch.equal(x.value()[0], y.value()[0]), what
        assert not torch.equal(x.value()[1], y.value()[1]), what
    img0 = lambda t: t.value().view(n, hw, c)[0]          # noqa: E731
    assert torch.equal(img0(a.out), img0(b.out))
    assert torch.equal(img0(ra[1]), img0(rb[1])) and torch.equal(img0(ra[2]), img0(rb[2]))


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _check_rc(rc, msg):
    err = _C.lib().tok_last_error()
    err = err.decode() if isinstance(err, bytes) else err
    assert rc == ERR_INVALID, (rc, err)
    assert msg in err, (msg, err)


@pytest.mark.parametrize('c,k,ld,null_z,msg', [(12, 3, 16, False, 'c % 8 == 0'), (2056, 3, 2056, False, 'c <= 2048'),
                                               (16, 4, 16, False, 'k odd'), (16, 17, 16, False, 'k <= 15'),
                                               (16, 3, 8, False, 'ld >= c'), (16, 3, 16, True, 'null pointer')])
def test_refusals(c, k, ld, null_z, msg):
    lib, st = _C.lib(), stream_ptr()
    n, hw = 2, 4
    rows = torch.zeros(n * hw * max(c, ld), dtype=BF, device='cuda')
    w = torch.zeros(32, device='cuda')
    mean, gate = torch.zeros(n * c, device='cuda'), torch.zeros(n * c, device='cuda')
    ws = torch.zeros(n * c * 4 + n * c + n * TAP_ROW, device='cuda')
    out, dz, ds, dw = torch.zeros_like(rows), torch.zeros_like(rows), torch.zeros_like(rows), torch.zeros(32, device='cuda')
    P = lambda t: t.data_ptr()        # noqa: E731
    z = None if null_z else P(rows)
    _check_rc(lib.tok_eca_fwd(z, P(rows), n, hw, c, ld, P(w), k, P(mean), P(gate), P(out), P(ws), st), 'tok_eca_fwd: ' + msg
              if null_z else msg)
    _check_rc(lib.tok_eca_bwd(P(rows), P(rows), z, n, hw, c, ld, P(w), k, P(mean), P(gate), P(dw), 0, P(dz), 0, P(ds), 0, P(ws),
                              st), 'tok_eca_bwd: ' + msg if null_z else msg)
    if c in (12, 2056):
        assert lib.tok_eca_ws_floats(n, hw, c) == 0
    torch.cuda.synchronize()
    assert not any(bool(t.any()) for t in (mean, gate, ws, out, dz, ds, dw))
