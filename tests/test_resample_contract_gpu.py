"""Kernel contract of the bilinear gather pair and the HRNet fuse pair (csrc/resample.hip, csrc/fuse_sum.hip), element by element against the fp64
reference of tests/resample_ref.py.  Operands sit in helpers.Guarded buffers: input pads and guard rows hold NaN, output pads
and guard rows hold sentinels that are checked after the call; the channels of dst outside [ch_off, ch_off + c) keep their
sentinel, the channels of ddst outside it hold NaN and no NaN reaches dsrc.

Two data sets.  INTEGERS in [-4, 4]: at a geometry whose weights are dyadic (resample_ref.dyadic on both axes: the factors
1, 2 and 8 of the table) every weight is a multiple of 1/16 per axis, every product a multiple of 2^-8 below 2^10 and every
fp32 partial sum exact in whatever order and with whatever contraction, so the result is BIT FOR BIT the fp64 result rounded
once to bf16.  The same for the fuse pair with scales in {1/4, 1/2, 1, 2} and integer shifts.  No tolerance there.

REALS, within helpers.assert_bounded: |got - ref| <= a |ref| + bound, with u = 2^-24 the fp32 unit roundoff:
  a = A_BF = 2^-8: the one rounding of the result to bf16 (2^-9 of the computed value; the factor 2 is slack that also
      covers 2^-9 of the computed value's own error).
  forward, bound = 7 u up_mag(x) + lam_term(x).  A tap's value reaches the result through two rounded weights (1 - lam per
      axis) and the four roundings of hy (hx a + lx b) + ly (hx c + lx d) (product, sum, product, sum; fewer when hipcc
      contracts): 6 u of up_mag = up64(|x|), second-order terms in the seventh.  lam_term is what the fp32 evaluation of the
      source coordinate does (|d lam| <= 3 u (s + 1) times the local slope |x[i1] - x[i0]|, derived in resample_ref).
  backward, bound = (T + 7) u (up_T_mag(g) + |previous|) + lam_term_T(g), T = the footprint of the transpose (taps per source
      pixel: resample_ref.taps_T of the two axes multiplied, from the reference's own weights).  A tap's weight carries at
      most 5 roundings (1 - lam and the sum of the two selected weights per axis, the product wy wx), the fma chain over the
      footprint at most T, the add of the previous value one; one more for second order.
  fuse forward, bound = (terms + 2) u sum_j repeat(|t_j| |sc_j| + |sf_j|): one rounding of the fma per term, at most `terms`
      additions, second order; relu is 1-Lipschitz and exact; plus 2^-133, the smallest bf16 subnormal, for a result that
      underflows (one channel of the all-affine reals is planted there: positive in fp32, stored as zero, and the mask
      must follow the stored value).  Backward, bound = (4^shift + 2) u (sum |dout| + |previous|).
The identity geometry is a bit copy (hy = hx = 1, the other taps times 0) for both data sets; a source no destination maps to
(the downsample) gets exactly +0 without `accumulate`.
"""
import pytest
import torch

import resample_ref as R
from helpers import A_BF, BF, ERR_INVALID, F32, SENTINEL, U8, U32, Guarded, assert_bounded, gin, gout, last_error, unpack_bits
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
ME = 'test_resample_contract_gpu'
BF_TINY = 2.0 ** -133      # the smallest bf16 subnormal: underflow of the stored result (the planted channel of test_fuse_forward)
# (hs, ws) -> (hd, wd)
SIZES = [((1, 1), (2, 2)), ((8, 8), (16, 16)), ((2, 4), (16, 32)), ((5, 7), (13, 20)), ((7, 5), (7, 10)), ((9, 9), (4, 5)),
         ((3, 3), (1, 1)), ((8, 8), (8, 8))]
# (c, ch_off, ld_src, ld_dst): three on the 16-byte path, two scalar by width, one scalar only because of the offset
CHANNELS = [(8, 0, 8, 8), (8, 24, 16, 40), (64, 24, 72, 96), (3, 5, 5, 11), (18, 18, 24, 56), (8, 4, 8, 16)]
BATCHES = (1, 3)


def _ids(v):
    return 'x'.join(str(i) for t in v for i in (t if isinstance(t, tuple) else (t,)))


def _bits(t):
    return t.contiguous().view(torch.int16)


def _bf16_of(ref64):
    """the fp64 result rounded once to bf16 (exact sums here are exact in fp32 too: no double rounding); -0 + 0 = +0"""
    return (ref64 + 0.0).to(BF)


def _data(shape, integers, g):
    return (torch.randint(-4, 5, shape, generator=g) if integers else torch.randn(shape, generator=g)).to(BF)


def _dyadic(size):
    (hs, ws), (hd, wd) = size
    return R.dyadic(hs, hd) and R.dyadic(ws, wd)


@pytest.mark.parametrize('chan', CHANNELS, ids=_ids)
@pytest.mark.parametrize('size', SIZES, ids=_ids)
def test_bilinear_forward(size, chan):
    (hs, ws), (hd, wd) = size
    c, ch_off, ld_src, ld_dst = chan
    lib, st = _C.lib(), stream_ptr()
    for n in BATCHES:
        for integers in (True, False):
            g = torch.Generator().manual_seed(hs * 131 + hd * 17 + c + n + 1000 * integers)
            x = _data((n, hs, ws, c), integers, g)
            src = Guarded(n * hs * ws, c, ld_src, init=x.cuda(), nan_pad=True)
            dst = Guarded(n * hd * wd, ld_dst)                                  # sentinels everywhere
            _C.check(lib.tok_bilinear_fwd(src.ptr, n, hs, ws, c, ld_src, dst.ptr, hd, wd, ld_dst, ch_off, st), 'tok_bilinear_fwd')
            torch.cuda.synchronize()
            what = f'dst n={n} integers={integers}'
            dst.check(what)
            full = dst.value().view(n, hd, wd, ld_dst)
            got = full[..., ch_off:ch_off + c]
            outside = _bits(torch.cat([full[..., :ch_off], full[..., ch_off + c:]], dim=-1))
            assert bool((outside == SENTINEL[BF]).all()), what + ': an element of dst outside the slice was written'
            ref = R.up64(x, (hd, wd))
            if (hs, ws) == (hd, wd):
                assert torch.equal(_bits(got), _bits(x)), what + ': the identity is not a bit copy'
            if integers and _dyadic(size):
                assert torch.equal(_bits(got), _bits(_bf16_of(ref))), what
            else:
                assert_bounded(got, ref, 7 * U32 * R.up_mag(x, (hd, wd)) + R.lam_term(x, (hd, wd)), A_BF, 1.0,
                               what=f'{_ids(size)}-{_ids(chan)} {what}', test=f'{ME}::test_bilinear_forward')


@pytest.mark.parametrize('chan', CHANNELS, ids=_ids)
@pytest.mark.parametrize('size', SIZES, ids=_ids)
def test_bilinear_backward(size, chan):
    (hs, ws), (hd, wd) = size
    c, ch_off, ld_src, ld_dst = chan
    lib, st = _C.lib(), stream_ptr()
    taps = R.taps_T(hs, hd) * R.taps_T(ws, wd)
    # sources no destination maps to, nor can reach through the fp32 evaluation of its coordinate
    empty = torch.outer((R.weight_matrix(hs, hd) + R.reach_matrix(hs, hd)).sum(0), (R.weight_matrix(ws, wd) + R.reach_matrix(ws, wd)).sum(0)) == 0
    assert bool((torch.outer(R.weight_matrix(hs, hd).sum(0), R.weight_matrix(ws, wd).sum(0)) == 0).any()) == (hd < hs or wd < ws)
    assert bool(empty.any()) == (size == ((9, 9), (4, 5)))            # (3 -> 1 lands on source 1 exactly: both neighbours are in reach)
    for n in BATCHES:
        for integers in (True, False):
            for accumulate in (0, 1):
                g = torch.Generator().manual_seed(hs * 131 + hd * 17 + c + n + 7 * accumulate + 1000 * integers)
                grad, prev = _data((n, hd, wd, c), integers, g), _data((n, hs, ws, c), integers, g)
                full = torch.full((n * hd * wd, ld_dst), float('nan'), dtype=BF)      # the other channels of ddst hold NaN
                full[:, ch_off:ch_off + c] = grad.view(-1, c)
                ddst = Guarded(n * hd * wd, ld_dst, init=full.cuda(), nan_pad=True)
                dsrc = Guarded(n * hs * ws, c, ld_src, init=prev.cuda() if accumulate else None)
                _C.check(lib.tok_bilinear_bwd(ddst.ptr, n, hd, wd, ld_dst, ch_off, dsrc.ptr, hs, ws, c, ld_src, accumulate, st),
                         'tok_bilinear_bwd')
                torch.cuda.synchronize()
                what = f'dsrc n={n} integers={integers} accumulate={accumulate}'
                dsrc.check(what)                                             # pad channels and guard row untouched
                got = dsrc.value().view(n, hs, ws, c)
                assert not bool(got.float().isnan().any()), what + ': a NaN of the other channels reached dsrc'
                start = prev if accumulate else torch.zeros_like(prev)
                ref = R.up64_T(grad, (hs, ws)) + start.double()
                if integers and _dyadic(size):
                    assert torch.equal(_bits(got), _bits(_bf16_of(ref))), what
                else:
                    mag = R.up_T_mag(grad, (hs, ws)) + start.double().abs()
                    assert_bounded(got, ref, (taps + 7) * U32 * mag + R.lam_term_T(grad, (hs, ws)), A_BF, 1.0,
                                   what=f'{_ids(size)}-{_ids(chan)} {what}', test=f'{ME}::test_bilinear_backward')
                if not accumulate:
                    assert bool((_bits(got[:, empty]) == 0).all()), what + ': empty preimage is not +0'


@pytest.mark.parametrize('size', [((5, 7), (13, 20)), ((9, 9), (4, 5))], ids=_ids)
def test_forward_and_backward_are_transposes_bit_for_bit(size):
    """The matrix of the forward (one-hot sources, the batch index as the one-hot position) and the matrix of the backward
    (one-hot gradients alike) have equal bits, entry by entry, in each of the 8 channels; both are bf16(wy wx) of the
    reference to within one bf16 ulp (A_BF w) once the fp32 evaluation of the weights is allowed for: d lam on every source a
    destination can reach (resample_ref) and the three roundings of 1 - lam per axis and of the product.  An entry out of
    reach has bound 0: it must be exactly zero.  (5 -> 13 holds the case that makes the allowance necessary: destination 6
    sits on source 2 exactly, the fp32 quotient puts it 4e-8 past it, and fp32 arithmetic rounds that away again.)"""
    (hs, ws), (hd, wd) = size
    c, ns, nd = 8, hs * ws, hd * wd
    lib, st = _C.lib(), stream_ptr()
    src = Guarded(ns * ns, c, init=torch.eye(ns).view(ns * ns, 1).expand(-1, c).to(BF).cuda(), nan_pad=True)
    dst = Guarded(ns * nd, c)
    _C.check(lib.tok_bilinear_fwd(src.ptr, ns, hs, ws, c, c, dst.ptr, hd, wd, c, 0, st), 'tok_bilinear_fwd')
    ddst = Guarded(nd * nd, c, init=torch.eye(nd).view(nd * nd, 1).expand(-1, c).to(BF).cuda(), nan_pad=True)
    dsrc = Guarded(nd * ns, c)
    _C.check(lib.tok_bilinear_bwd(ddst.ptr, nd, hd, wd, c, 0, dsrc.ptr, hs, ws, c, c, 0, st), 'tok_bilinear_bwd')
    torch.cuda.synchronize()
    dst.check('dst')
    dsrc.check('dsrc')
    fwd = dst.value().view(ns, nd, c)                 # [source][destination]
    bwd = dsrc.value().view(nd, ns, c)                # [destination][source]
    assert torch.equal(_bits(fwd), _bits(bwd.transpose(0, 1)))
    wy, wx = R.weight_matrix(hs, hd), R.weight_matrix(ws, wd)
    w = torch.einsum('da,eb->abde', wy, wx).reshape(ns, nd)
    # where the kernels' fp32 weights may lie: d lam of one axis times the weight of the other, on every source in reach
    reach = (torch.einsum('da,eb->abde', R.reach_matrix(hs, hd), wx) + torch.einsum('da,eb->abde', wy, R.reach_matrix(ws, wd))).reshape(ns, nd)
    for ch in range(c):
        assert_bounded(fwd[..., ch], w, reach + 3 * U32 * w, A_BF, 1.0, what=f'{_ids(size)} matrix, channel {ch}')


def test_offsets_past_2_31_elements():
    """dst [1][2048][2048][520], c = 8 at ch_off = 512 from 1024 x 1024: 2.18e9 elements, the slice of the last rows starts
    past 2^31.  Factor 2 on integers: bit for bit.  Forward on the last 8 rows and 8 rows in the middle against the reference
    evaluated on the device from slices; backward of an all-ones gradient = the outer product of the weights' column sums,
    4 in the interior and whatever the reference gives on the border (the clamp returns the mass that falls off the edge)."""
    n, hs, ws, c, hd, wd, ld, off = 1, 1024, 1024, 8, 2048, 2048, 520, 512
    assert n * hd * wd * ld > 2 ** 31
    lib, st = _C.lib(), stream_ptr()
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-4, 5, (n, hs, ws, c), generator=g).to(BF).cuda()
    dst = torch.empty((n, hd, wd, ld), dtype=BF, device='cuda')
    bands = ((2040, 2048), (1020, 1028))
    for lo, hi in bands:
        dst[0, lo:hi, :, off:off + c] = 100.0
    _C.check(lib.tok_bilinear_fwd(x.data_ptr(), n, hs, ws, c, c, dst.data_ptr(), hd, wd, ld, off, st), 'tok_bilinear_fwd')
    for lo, hi in bands:
        want = R.up64(x, (hd, wd), rows=(lo, hi)).to(BF)
        assert torch.equal(_bits(dst[:, lo:hi, :, off:off + c]), _bits(want)), (lo, hi)
    dst[..., off:off + c] = 1.0
    dsrc = torch.empty_like(x)
    _C.check(lib.tok_bilinear_bwd(dst.data_ptr(), n, hd, wd, ld, off, dsrc.data_ptr(), hs, ws, c, c, 0, st), 'tok_bilinear_bwd')
    torch.cuda.synchronize()
    col = R.weight_matrix(hs, hd).sum(0)
    want = torch.outer(col, col)                       # hs == ws, hd == wd
    assert bool((want[1:-1, 1:-1] == 4).all())
    assert torch.equal(dsrc.double().cpu(), want.view(1, hs, ws, 1).expand(-1, -1, -1, c))


_OK = dict(n=2, hs=3, ws=2, c=8, ld_src=8, hd=6, wd=4, ld_dst=16, ch_off=8)
_BAD = [dict(n=0), dict(hs=0), dict(ws=-1), dict(c=0), dict(hd=0), dict(wd=-2), dict(c=16, ld_dst=32), dict(ch_off=-8),
        dict(ch_off=16), dict(c=8, ch_off=9), dict(src=None), dict(dst=None)]


@pytest.mark.parametrize('bad', _BAD, ids=lambda d: ','.join(f'{k}={v}' for k, v in d.items()))
def test_bilinear_refusals(bad):
    """a non-positive extent, c > ld_src, ch_off < 0, ch_off + c > ld_dst, a null pointer: the invalid-argument code, the
    message in tok_last_error, and nothing written"""
    lib, st = _C.lib(), stream_ptr()
    a = dict(_OK, **{k: v for k, v in bad.items() if k not in ('src', 'dst')})
    small = Guarded(a['n'] * a['hs'] * a['ws'] if min(a['n'], a['hs'], a['ws']) > 0 else 1, 8, 8)
    big = Guarded(a['n'] * a['hd'] * a['wd'] if min(a['n'], a['hd'], a['wd']) > 0 else 1, 16, 16)
    sp = None if 'src' in bad else small.ptr
    dp = None if 'dst' in bad else big.ptr
    rc = lib.tok_bilinear_fwd(sp, a['n'], a['hs'], a['ws'], a['c'], a['ld_src'], dp, a['hd'], a['wd'], a['ld_dst'], a['ch_off'], st)
    assert rc == ERR_INVALID and 'tok_bilinear_fwd: bad args' in last_error()
    for accumulate in (0, 1):
        rc = lib.tok_bilinear_bwd(dp, a['n'], a['hd'], a['wd'], a['ld_dst'], a['ch_off'], sp, a['hs'], a['ws'], a['c'], a['ld_src'],
                                  accumulate, st)
        assert rc == ERR_INVALID and 'tok_bilinear_bwd: bad args' in last_error()
    torch.cuda.synchronize()
    for buf in (small, big):
        buf.check('refused call')
        assert bool((_bits(buf.view) == SENTINEL[BF]).all())


# ---- HRNet fuse sum ---------------------------------------------------------------------------------------------------------------
FUSE = [(2, 16, 16, 16, (0, 1, 2, 3)), (2, 8, 24, 48, (0, 0, 1)), (1, 8, 8, 8, (0,)), (3, 8, 8, 64, (0, 2))]
AFFINE = {'none': lambda j: False, 'all': lambda j: True, 'mixed': lambda j: j % 2 == 0}


def _fuse_id(v):
    return _ids(v[:4]) + '-s' + ''.join(str(s) for s in v[4])


@pytest.mark.parametrize('pattern', list(AFFINE))
@pytest.mark.parametrize('relu', (0, 1))
@pytest.mark.parametrize('shape', FUSE, ids=_fuse_id)
def test_fuse_forward(shape, relu, pattern):
    n, h, w, c, shifts = shape
    lib, st = _C.lib(), stream_ptr()
    for integers in (True, False):
        g = torch.Generator().manual_seed(h * 7 + c + relu + 1000 * integers)
        terms = [_data((n, h >> s, w >> s, c), integers, g) for s in shifts]
        scs, sfs = [], []
        for j in range(len(shifts)):
            if not AFFINE[pattern](j):
                scs.append(None)
                sfs.append(None)
            elif integers:
                scs.append(torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (c,), generator=g)])
                sfs.append(torch.randint(-3, 4, (c,), generator=g).float())
            else:
                scs.append(torch.rand(c, generator=g) + 0.5)
                sfs.append(torch.randn(c, generator=g))
        if not integers and pattern == 'all':
            # channel 0 of every term scaled by 2^-140 (an fp32 subnormal): the sums are positive in fp32 about half the time,
            # yet below half the smallest bf16 subnormal, so they are STORED as zero — and the mask follows what is stored
            for sc, sf in zip(scs, sfs):
                sc[0], sf[0] = 2.0 ** -140, 0.0
        tb = [Guarded(t.numel() // c, c, init=t.cuda(), nan_pad=True) for t in terms]
        cb = [None if v is None else gin(v.cuda(), 64) for v in scs]
        fb = [None if v is None else gin(v.cuda(), 64) for v in sfs]
        out = Guarded(n * h * w, c)
        mask = gout(n * h * w * c // 8, U8, 256)
        out2 = Guarded(n * h * w, c)
        for o, m in ((out, mask.ptr), (out2, None)):             # mask = NULL: the sum alone
            if pattern == 'none':
                a = []
                for j in range(4):
                    a += [tb[j].ptr, shifts[j]] if j < len(terms) else [None, 0]
                _C.check(lib.tok_fuse_sum_relu_fwd(*a, n, h, w, c, relu, o.ptr, m, st), 'tok_fuse_sum_relu_fwd')
            else:
                a = []
                for j in range(4):
                    a += ([tb[j].ptr, shifts[j], cb[j] and cb[j].ptr, fb[j] and fb[j].ptr] if j < len(terms) else [None, 0, None, None])
                _C.check(lib.tok_fuse_sum_affine_relu_fwd(*a, n, h, w, c, relu, o.ptr, m, st), 'tok_fuse_sum_affine_relu_fwd')
        torch.cuda.synchronize()
        what = f'{_fuse_id(shape)} relu={relu} {pattern} integers={integers}'
        out.check(what)
        out2.check(what)
        mask.check(what)
        got, mbytes = out.value().view(n, h, w, c), mask.value().view(n * h * w, c // 8)
        assert torch.equal(_bits(out2.value()), _bits(out.value())), what + ': mask = NULL changes the sum'
        # the mask is `stored out > 0`, on every element, relu or not
        assert torch.equal(mbytes, R.fuse_mask(got)), what + ': a mask bit is not (stored out > 0)'
        ref = R.fuse64(terms, shifts, scs, sfs, relu)
        if integers:
            want = _bf16_of(ref)
            assert torch.equal(_bits(got), _bits(want)), what
            assert torch.equal(mbytes, R.fuse_mask(want)), what
        else:
            mag = R.fuse64(terms, shifts, scs, sfs, relu, absolute=True)
            assert_bounded(got, ref, (len(shifts) + 2) * U32 * mag + BF_TINY, A_BF, 1.0, what=what, test=f'{ME}::test_fuse_forward')


@pytest.mark.parametrize('shape', FUSE, ids=_fuse_id)
def test_fuse_backward(shape):
    n, h, w, c, shifts = shape
    lib, st = _C.lib(), stream_ptr()
    for s in sorted(set(shifts)):
        hs, ws = h >> s, w >> s
        for integers in (True, False):
            for accumulate in (0, 1):
                for masked in (True, False):
                    g = torch.Generator().manual_seed(h * 7 + c + s + 10 * accumulate + 1000 * integers)
                    grad, prev = _data((n, h, w, c), integers, g), _data((n, hs, ws, c), integers, g)
                    mbytes = torch.randint(0, 256, (n * h * w, c // 8), generator=g).to(U8)
                    keep = unpack_bits(mbytes, n * h * w, c).view(n, h, w, c) if masked else None
                    dout = Guarded(n * h * w, c, init=grad.cuda(), nan_pad=True)
                    mask = gin(mbytes.cuda(), 256)
                    dterm = Guarded(n * hs * ws, c, init=prev.cuda() if accumulate else None)
                    _C.check(lib.tok_fuse_sum_relu_bwd(dout.ptr, mask.ptr if masked else None, n, h, w, c, s, dterm.ptr, accumulate, st),
                             'tok_fuse_sum_relu_bwd')
                    torch.cuda.synchronize()
                    what = f'{_fuse_id(shape)} shift={s} integers={integers} accumulate={accumulate} masked={masked}'
                    dterm.check(what)
                    got = dterm.value().view(n, hs, ws, c)
                    start = prev if accumulate else None
                    ref = R.fuse_T64(grad, keep, s, start)
                    if integers:      # |sum| <= 64 * 4 + 4: exact in fp32, rounded once
                        assert torch.equal(_bits(got), _bits(_bf16_of(ref))), what
                    else:
                        assert_bounded(got, ref, R.fuse_T64(grad, keep, s, start, absolute=True), A_BF, (4 ** s + 2) * U32, what=what,
                                       test=f'{ME}::test_fuse_backward')


_FUSE_OK = dict(n=1, h=8, w=8, c=8, s0=0, s1=1, t0=True, t1=True, sc0=False, sf0=False, out=True)
_FUSE_BAD = [(dict(n=0), 'bad args'), (dict(h=0), 'bad args'), (dict(w=-8), 'bad args'), (dict(c=0), 'bad args'), (dict(c=12), 'bad args'),
             (dict(out=False), 'bad args'), (dict(t0=False, t1=False), 'bad args'),
             (dict(h=12, w=12, s1=3), 'term 1: 12x12 is not a multiple of 2^3'), (dict(h=8, w=10, s1=2), 'term 1: 8x10 is not a multiple of 2^2'),
             (dict(s1=8), 'term 1: 8x8 is not a multiple of 2^8'), (dict(s0=-1), 'term 0: 8x8 is not a multiple of 2^-1'),
             (dict(sc0=True), 'term 0: scale without shift'), (dict(sf0=True), 'term 0: scale without shift')]


@pytest.mark.parametrize('bad,msg', _FUSE_BAD, ids=lambda v: ','.join(f'{k}={x}' for k, x in v.items()) if isinstance(v, dict) else None)
def test_fuse_forward_refusals(bad, msg):
    """non-positive extents, c % 8 != 0, a null out, no term at all, a map that is no multiple of 2^shift, a shift outside
    [0, 8), a scale without its shift and a shift without its scale: invalid-argument code, message, nothing written"""
    lib, st = _C.lib(), stream_ptr()
    a = dict(_FUSE_OK, **bad)
    rows = 16 * 16
    t0, t1, out = Guarded(rows, 16), Guarded(rows, 16), Guarded(rows, 16)
    coef, mask = gout(16, F32, 64), gout(rows * 2, U8, 256)
    t0p, t1p = (t0.ptr if a['t0'] else None), (t1.ptr if a['t1'] else None)
    affine = a['sc0'] or a['sf0']
    if not affine:
        rc = lib.tok_fuse_sum_relu_fwd(t0p, a['s0'], t1p, a['s1'], None, 0, None, 0, a['n'], a['h'], a['w'], a['c'], 1,
                                       out.ptr if a['out'] else None, mask.ptr, st)
        assert rc == ERR_INVALID and last_error() == 'tok_fuse_sum_relu_fwd: ' + msg
    rc = lib.tok_fuse_sum_affine_relu_fwd(t0p, a['s0'], coef.ptr if a['sc0'] else None, coef.ptr if a['sf0'] else None, t1p, a['s1'], None, None,
                                          None, 0, None, None, None, 0, None, None, a['n'], a['h'], a['w'], a['c'], 1,
                                          out.ptr if a['out'] else None, mask.ptr, st)
    assert rc == ERR_INVALID and last_error() == 'tok_fuse_sum_relu_fwd: ' + msg
    torch.cuda.synchronize()
    for buf in (t0, t1, out):
        buf.check('refused call')
        assert bool((_bits(buf.view) == SENTINEL[BF]).all())
    mask.check('refused call')
    assert mask.untouched() and coef.untouched()


_FUSE_BWD_BAD = [dict(n=0), dict(h=-8), dict(w=0), dict(c=0), dict(c=12), dict(shift=8), dict(shift=-1), dict(h=12, w=12, shift=3),
                 dict(h=8, w=10, shift=2), dict(dout=None), dict(dterm=None)]


@pytest.mark.parametrize('bad', _FUSE_BWD_BAD, ids=lambda d: ','.join(f'{k}={v}' for k, v in d.items()))
def test_fuse_backward_refusals(bad):
    lib, st = _C.lib(), stream_ptr()
    a = dict(dict(n=1, h=8, w=8, c=8, shift=1), **{k: v for k, v in bad.items() if k not in ('dout', 'dterm')})
    dout, dterm = Guarded(16 * 16, 16), Guarded(16 * 16, 16)
    mask = gout(16 * 16 * 2, U8, 256)
    for accumulate in (0, 1):
        for m in (mask.ptr, None):
            rc = lib.tok_fuse_sum_relu_bwd(None if 'dout' in bad else dout.ptr, m, a['n'], a['h'], a['w'], a['c'], a['shift'],
                                           None if 'dterm' in bad else dterm.ptr, accumulate, st)
            assert rc == ERR_INVALID and last_error() == 'tok_fuse_sum_relu_bwd: bad args'
    torch.cuda.synchronize()
    for buf in (dout, dterm):
        buf.check('refused call')
        assert bool((_bits(buf.view) == SENTINEL[BF]).all())
    assert mask.untouched()
