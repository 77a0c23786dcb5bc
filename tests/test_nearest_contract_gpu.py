"""Kernel contract of tok_nearest_fwd/_bwd (csrc/resample.hip), element by element.  The forward is a copy: bit for bit
F.interpolate(mode='nearest') of the source, placed at ch_off, every other element of dst untouched.  The backward is its
transpose: bit for bit the fp64 transpose on small-integer gradients (the sums are exact), within one bf16 rounding of the
result plus the fp32 accumulation on reals, with and without `accumulate`; sources no destination maps to get exact zeros;
the pad channels of dsrc stay untouched.  Operands sit in helpers.Guarded buffers: input pads and guard rows hold NaN, output
pads and guard rows hold sentinels that are checked after the call."""
import pytest
import torch
import torch.nn.functional as F

from helpers import BF, ERR_INVALID, SENTINEL, Guarded, assert_bounded, last_error
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
A_BF, B_BF = 2.0 ** -8, 2.0 ** -16    # bf16 result accumulated in fp32 (tests/test_dwconv_se_contract_gpu.py)
# (hs, ws) -> (hd, wd): x2 of one pixel, x2, height only, a non-integer ratio, the identity, a downsample (empty preimages)
SIZES = [((1, 1), (2, 2)), ((3, 2), (6, 4)), ((5, 4), (6, 4)), ((7, 5), (13, 9)), ((9, 7), (9, 7)), ((6, 4), (3, 2))]
# (c, ch_off, ld_src, ld_dst): the first four take the 16-byte path, the last two (odd widths, offsets, pitches) the scalar one
CHANNELS = [(8, 0, 8, 8), (8, 24, 16, 40), (64, 0, 64, 64), (64, 24, 72, 96), (3, 5, 5, 11), (18, 5, 19, 27)]
BATCHES = (1, 3)


def _src_index(s, d):
    """the source index of every destination index, from torch itself"""
    return F.interpolate(torch.arange(s, dtype=torch.float32).view(1, 1, s, 1), size=(d, 1), mode='nearest').view(-1).long()


def _ids(v):
    return 'x'.join(str(i) for t in v for i in (t if isinstance(t, tuple) else (t,)))


@pytest.mark.parametrize('chan', CHANNELS, ids=_ids)
@pytest.mark.parametrize('size', SIZES, ids=_ids)
def test_forward_is_the_interpolated_copy(size, chan):
    (hs, ws), (hd, wd) = size
    c, ch_off, ld_src, ld_dst = chan
    lib, st = _C.lib(), stream_ptr()
    for n in BATCHES:
        g = torch.Generator().manual_seed(hs * 131 + hd * 17 + c + n)
        x = torch.randn(n, hs, ws, c, generator=g).to(BF)
        src = Guarded(n * hs * ws, c, ld_src, init=x.cuda(), nan_pad=True)
        dst = Guarded(n * hd * wd, ld_dst)                                  # sentinels everywhere
        _C.check(lib.tok_nearest_fwd(src.ptr, n, hs, ws, c, ld_src, dst.ptr, hd, wd, ld_dst, ch_off, st), 'tok_nearest_fwd')
        torch.cuda.synchronize()
        dst.check(f'dst n={n}')
        want = F.interpolate(x.float().permute(0, 3, 1, 2), size=(hd, wd), mode='nearest').permute(0, 2, 3, 1).to(BF)
        got = dst.value().view(n, hd, wd, ld_dst)
        assert torch.equal(got[..., ch_off:ch_off + c].view(torch.int16), want.view(torch.int16)), n
        outside = torch.cat([got[..., :ch_off], got[..., ch_off + c:]], dim=-1).view(torch.int16)
        assert bool((outside == SENTINEL[BF]).all()), f'n={n}: an element of dst outside the slice was written'


def _transpose64(g, prev, hs, ws):
    """fp64 transpose of the forward: prev + the sum of g over every destination pixel that maps to the source pixel"""
    n, hd, wd, c = g.shape
    rows = torch.zeros(n, hs, wd, c, dtype=torch.float64).index_add_(1, _src_index(hs, hd), g.double())
    return prev.double().index_add(2, _src_index(ws, wd), rows)


@pytest.mark.parametrize('chan', CHANNELS, ids=_ids)
@pytest.mark.parametrize('size', SIZES, ids=_ids)
def test_backward_is_the_transpose(size, chan):
    (hs, ws), (hd, wd) = size
    c, ch_off, ld_src, ld_dst = chan
    lib, st = _C.lib(), stream_ptr()
    iy, ix = _src_index(hs, hd), _src_index(ws, wd)
    empty = torch.ones(hs, ws, dtype=torch.bool)
    empty[iy[:, None], ix[None, :]] = False                                  # sources no destination maps to
    assert bool(empty.any()) == (hd < hs)
    for n in BATCHES:
        for integers in (True, False):
            for accumulate in (0, 1):
                g = torch.Generator().manual_seed(hs * 131 + hd * 17 + c + n + 7 * accumulate)
                if integers:      # |sum| <= 4 * 4 + 4 < 256: every partial sum and the result are exact in bf16
                    grad = torch.randint(-4, 5, (n, hd, wd, c), generator=g).to(BF)
                    prev = torch.randint(-4, 5, (n, hs, ws, c), generator=g).to(BF)
                else:
                    grad = torch.randn(n, hd, wd, c, generator=g).to(BF)
                    prev = torch.randn(n, hs, ws, c, generator=g).to(BF)
                full = torch.full((n * hd * wd, ld_dst), float('nan'), dtype=BF)      # the other channels of ddst hold NaN
                full[:, ch_off:ch_off + c] = grad.view(-1, c)
                ddst = Guarded(n * hd * wd, ld_dst, init=full.cuda(), nan_pad=True)
                dsrc = Guarded(n * hs * ws, c, ld_src, init=prev.cuda() if accumulate else None)
                _C.check(lib.tok_nearest_bwd(ddst.ptr, n, hd, wd, ld_dst, ch_off, dsrc.ptr, hs, ws, c, ld_src, accumulate, st),
                         'tok_nearest_bwd')
                torch.cuda.synchronize()
                what = f'dsrc n={n} integers={integers} accumulate={accumulate}'
                dsrc.check(what)                                             # pad channels and guard row untouched
                got = dsrc.value().view(n, hs, ws, c)
                start = prev if accumulate else torch.zeros_like(prev)
                ref = _transpose64(grad, start, hs, ws)
                if integers:
                    assert torch.equal(got.double(), ref), what
                else:
                    assert_bounded(got, ref, _transpose64(grad.abs(), start.abs(), hs, ws), A_BF, B_BF,
                                   what=f'{_ids(size)}-{_ids(chan)} {what}', test='test_nearest_contract_gpu::test_backward_is_the_transpose')
                if not accumulate:
                    assert bool((got[:, empty].view(torch.int16) == 0).all()), what + ': empty preimage is not +0'


def test_offsets_past_2_31_elements():
    """dst [1][2048][2048][520]: 2.18e9 elements, the smallest such shape at which a 32-bit element offset goes wrong (the
    slice of the last rows starts past 2^31).  Forward checked on the last 8 rows and 8 rows near the middle; the transpose of
    what the forward wrote is 4 x the source exactly (four equal terms), checked everywhere."""
    n, hs, ws, c, hd, wd, ld, off = 1, 1024, 1024, 8, 2048, 2048, 520, 512
    assert n * hd * wd * ld > 2 ** 31
    lib, st = _C.lib(), stream_ptr()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, hs, ws, c, generator=g).to(BF).cuda()
    dst = torch.empty((n, hd, wd, ld), dtype=BF, device='cuda')
    dst[0, 2040:, :, off:off + c] = 0
    dst[0, 1020:1028, :, off:off + c] = 0
    _C.check(lib.tok_nearest_fwd(x.data_ptr(), n, hs, ws, c, c, dst.data_ptr(), hd, wd, ld, off, st), 'tok_nearest_fwd')
    iy, ix = _src_index(hs, hd).cuda(), _src_index(ws, wd).cuda()
    for lo, hi in ((2040, 2048), (1020, 1028)):
        want = x[0][iy[lo:hi]][:, ix]
        assert torch.equal(dst[0, lo:hi, :, off:off + c].view(torch.int16), want.view(torch.int16)), (lo, hi)
    dsrc = torch.empty_like(x)
    _C.check(lib.tok_nearest_bwd(dst.data_ptr(), n, hd, wd, ld, off, dsrc.data_ptr(), hs, ws, c, c, 0, st), 'tok_nearest_bwd')
    torch.cuda.synchronize()
    assert torch.equal(dsrc.float(), 4 * x.float())


_OK = dict(n=2, hs=3, ws=2, c=8, ld_src=8, hd=6, wd=4, ld_dst=16, ch_off=8)
_BAD = [dict(n=0), dict(hs=0), dict(ws=-1), dict(c=0), dict(hd=0), dict(wd=0), dict(c=16, ld_dst=32), dict(ch_off=-8),
        dict(ch_off=16), dict(c=8, ch_off=9), dict(src=None), dict(dst=None)]


@pytest.mark.parametrize('bad', _BAD, ids=lambda d: ','.join(f'{k}={v}' for k, v in d.items()))
def test_refusals(bad):
    """a non-positive extent, c > ld_src, ch_off < 0, ch_off + c > ld_dst, a null pointer: the invalid-argument code, the
    message in tok_last_error, and nothing written"""
    lib, st = _C.lib(), stream_ptr()
    a = dict(_OK, **{k: v for k, v in bad.items() if k not in ('src', 'dst')})
    small = Guarded(a['n'] * a['hs'] * a['ws'] if min(a['n'], a['hs'], a['ws']) > 0 else 1, 8, 8)
    big = Guarded(a['n'] * a['hd'] * a['wd'] if min(a['n'], a['hd'], a['wd']) > 0 else 1, 16, 16)
    sp = None if 'src' in bad else small.ptr
    dp = None if 'dst' in bad else big.ptr
    rc = lib.tok_nearest_fwd(sp, a['n'], a['hs'], a['ws'], a['c'], a['ld_src'], dp, a['hd'], a['wd'], a['ld_dst'], a['ch_off'], st)
    assert rc == ERR_INVALID and 'tok_nearest_fwd: bad args' in last_error()
    rc = lib.tok_nearest_bwd(dp, a['n'], a['hd'], a['wd'], a['ld_dst'], a['ch_off'], sp, a['hs'], a['ws'], a['c'], a['ld_src'], 0, st)
    assert rc == ERR_INVALID and 'tok_nearest_bwd: bad args' in last_error()
    torch.cuda.synchronize()
    for buf in (small, big):
        buf.check('refused call')
        assert bool((buf.view.view(torch.int16) == SENTINEL[BF]).all())
