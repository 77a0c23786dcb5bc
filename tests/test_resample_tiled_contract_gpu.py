"""Kernel contract of tok_bilinear_sum_stats and tok_bilinear_bwd_multi (csrc/neck_resample.hip: the tiled LDS kernels of the commuted
HRNet neck and the generic kernels behind them), element by element against the fp64 reference of tests/resample_ref.py — not
against tok_bilinear_bwd, which shares src_index with them.

Which kernel runs is the launcher's rule, restated here as `tiled_rule`: c % 8 == 0, the map a multiple of 16, every source an
exact factor 2, 4 or 8 in both axes, at most one source per factor, and the tile count within the grid limit (65536 workgroups
for the sum, 2^31 - 1 for the transpose).  Every case records which kernel the rule selects; the TILED table holds the
smallest shapes that reach each mechanism of the tiled kernels, the FALLBACK table tiled-looking shapes that must take the
generic path.

Operands sit in helpers.GuardedSpan buffers, a guard in front and one behind (the tiled kernels stage halos that reach
backwards): NaN around inputs, sentinels around outputs, checked after the call.  Outputs start as sentinels, so an element
the kernel does not write shows.

INTEGERS in [-4, 4] at power-of-two factors: weights are multiples of 1/(2F) per axis, products multiples of 2^-8 (2^-10 at
factor 16), the largest footprint of the transpose holds 16 x 16 taps with weights summing to 64, so |sum| <= 256 and every
fp32 partial sum is exact in any order: the outputs are BIT FOR BIT the fp64 result rounded once to bf16.

REALS within helpers.assert_bounded, a = A_BF = 2^-8 (the one rounding to bf16), u = 2^-24:
  sum: bound = 13 u (|y0| + sum_j up_mag(t_j)) + sum_j lam_term(t_j).  13 = 1 + 3 * 4 is the number of terms of the sum, and
      no term passes more roundings than that in either kernel: two rounded weights (1 - lam per axis), four roundings of the
      blend (tiled: hx a + lx b, then wa X + wb X'; generic: blend4), at most three additions of sources = 9, the rest covers
      second order.  lam_term as in resample_ref (zero effect at the factors 2 / 4 / 8, where s is exact in fp32).
  transpose: bound = (T + 7) u up_T_mag(g) + lam_term_T(g), T = the footprint from the reference's weights ((2F)^2 in the
      interior), as for tok_bilinear_bwd (tests/test_resample_contract_gpu.py); the tiled kernel adds a row of 2F taps, then
      its rows, then folds row parts with shuffles — fewer than T roundings on any path.
  partial rows, tiled form: row r = (sum, sum of squares) of the stored bf16 y over the 256 pixels of tile r per channel,
      compared with fp64 sums of the kernel's own stored output (which the checks above have tied to the reference).  The fold
      read in the kernel: a lane adds its four rows in order (3 roundings, the first add to zero is exact), the 16 lanes of a
      channel group fold by a 4-level xor butterfly, the four waves are added in wave order (3): every value passes at most
      10 additions — a tree bound, 11 u with second order, well inside the 256 u of a sequential sum over the tile.  The
      squares f * f of bf16 values are exact in fp32.  Bounds: 11 u sum |f| and 11 u sum f^2.
  partial rows, generic form: only the fold over the rows is defined (a lane adds its rows in stride order, the row lanes in
      order, the test folds the rows in fp64): bound M u sum |f| and M u sum f^2, M = n h w elements per channel.
"""
import itertools

import pytest
import torch

import resample_ref as R
from helpers import A_BF, BF, ERR_INVALID, F32, U32, assert_bounded, gin, gout, last_error
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
ME = 'test_resample_tiled_contract_gpu'
GUARD = 4096
SUM_GRID, ADJ_GRID = 65536, 2 ** 31 - 1


def tiled_rule(n, h, w, c, lows, grid_limit):
    if c % 8 or h % 16 or w % 16 or n * (h // 16) * (w // 16) > grid_limit:
        return False
    seen = set()
    for hs, ws in lows:
        f = h // hs
        if f not in (2, 4, 8) or hs * f != h or ws * f != w or f in seen:
            return False
        seen.add(f)
    return True


def _by_factor(h, w, factors):
    return [(h // f, w // f) for f in factors]


# (n, h, w, c, sources (hs, ws) in argument order, tiled?)
TILED = ([(1, 16, 16, 8, _by_factor(16, 16, (2, 4, 8)), True),          # one tile, all four borders, a chunk with one live group of four
          (2, 48, 48, 40, _by_factor(48, 48, (8, 2, 4)), True),         # a tile with neighbours on all sides, batch stride, 1 1/4 chunks
          (1, 16, 32, 32, _by_factor(16, 32, (2, 4, 8)), True)] +       # exactly one full chunk, non-square
         [(1, 32, 16, 72, _by_factor(32, 16, f), True)                  # nine groups: three trips through the prefetch pipeline
          for k in (1, 2) for f in itertools.combinations((2, 4, 8), k)])
FALLBACK = [(1, 32, 32, 16, [(16, 16), (16, 16)], False),               # two sources of one factor
            (1, 32, 32, 16, [(11, 11)], False),                         # non-integer factor
            (1, 32, 32, 16, [(16, 8)], False),                          # factor 2 down, 4 across
            (1, 32, 32, 8, [(2, 2)], False),                            # factor 16
            (1, 24, 24, 8, [(12, 12), (6, 6), (3, 3)], False),          # map not a multiple of 16
            (2, 13, 20, 24, [(5, 7)], False),                           # map not a multiple of 16
            (1, 8, 8, 2056, [(4, 4)], False)]                           # a lane walks several channel groups
SUM_CASES = TILED + [(3, 16, 16, 8, [], True)] + FALLBACK               # no sources: the tiled kernel copies and counts
ADJ_CASES = TILED + FALLBACK + [(1, 16, 16, 12, [(8, 8)], False)]       # scalar gather


def _case_id(v):
    n, h, w, c, lows, tiled = v
    return f'{n}x{h}x{w}x{c}-' + ('_'.join(f'{a}x{b}' for a, b in lows) or 'none') + ('-tiled' if tiled else '-generic')


def _bits(t):
    return t.contiguous().view(torch.int16)


def _bf16_of(ref64):
    return (ref64 + 0.0).to(BF)


def _data(shape, integers, g):
    return (torch.randint(-4, 5, shape, generator=g) if integers else torch.randn(shape, generator=g)).to(BF)


def _all_dyadic(h, w, lows):
    return all(R.dyadic(hs, h) and R.dyadic(ws, w) for hs, ws in lows)


def _sum_args(y0p, srcs, lows, n, h, w, c, yp, statsp):
    a = [y0p]
    for j in range(3):
        a += [srcs[j].ptr, lows[j][0], lows[j][1]] if j < len(lows) else [None, 1, 1]
    return a + [n, h, w, c, yp, statsp, stream_ptr()]


def _tile_sums(f, n, h, w, c):
    """[n tiles_y tiles_x][c] sums of f [n][h][w][c] over 16 x 16 tiles, in the kernel's tile order"""
    return f.view(n, h // 16, 16, w // 16, 16, c).sum(dim=(2, 4)).reshape(-1, c)


def _check_stats(part, y_stored, n, h, w, c, rows, tiled, what):
    f = y_stored.double().view(n, h, w, c)
    if tiled:
        assert rows == n * (h // 16) * (w // 16)
        assert_bounded(part[0], _tile_sums(f, n, h, w, c), _tile_sums(f.abs(), n, h, w, c), 0.0, 11 * U32, what + ' tile sums', f'{ME}::stats')
        assert_bounded(part[1], _tile_sums(f * f, n, h, w, c), _tile_sums(f * f, n, h, w, c), 0.0, 11 * U32, what + ' tile squares', f'{ME}::stats')
    else:
        m = n * h * w
        f = f.view(m, c)
        assert_bounded(part[0].sum(0), f.sum(0), f.abs().sum(0), 0.0, m * U32, what + ' folded sums', f'{ME}::stats')
        assert_bounded(part[1].sum(0), (f * f).sum(0), (f * f).sum(0), 0.0, m * U32, what + ' folded squares', f'{ME}::stats')


@pytest.mark.parametrize('case', SUM_CASES, ids=_case_id)
def test_sum_stats(case):
    n, h, w, c, lows, tiled = case
    assert tiled_rule(n, h, w, c, lows, SUM_GRID) == tiled
    lib = _C.lib()
    rows = lib.tok_bilinear_sum_stats_rows(n, h, w, c)
    assert rows >= 1
    for integers in ((True, False) if _all_dyadic(h, w, lows) else (False,)):
        g = torch.Generator().manual_seed(h * 13 + c + len(lows) + 1000 * integers)
        y0 = _data((n, h, w, c), integers, g)
        ts = [_data((n, hs, ws, c), integers, g) for hs, ws in lows]
        ref = y0.double()
        mag = y0.double().abs()
        lam = torch.zeros_like(ref)
        for t in ts:
            ref = ref + R.up64(t, (h, w))
            mag = mag + R.up_mag(t, (h, w))
            lam = lam + R.lam_term(t, (h, w))
        srcs = [gin(t.cuda(), GUARD) for t in ts]
        runs = {}
        for mode in ('in place', 'out of place', 'no stats'):
            what = f'{_case_id(case)} integers={integers} {mode}'
            y = gout(y0.numel(), BF, GUARD, init=y0.cuda() if mode == 'in place' else None)
            y0b = y if mode == 'in place' else gin(y0.cuda(), GUARD)
            stats = gout(2 * rows * c, F32, GUARD)
            _C.check(lib.tok_bilinear_sum_stats(*_sum_args(y0b.ptr, srcs, lows, n, h, w, c, y.ptr, None if mode == 'no stats' else stats.ptr)),
                     'tok_bilinear_sum_stats')
            torch.cuda.synchronize()
            for buf in (y, y0b, stats):
                buf.check(what)
            if mode == 'out of place':
                assert torch.equal(_bits(y0b.value()), _bits(y0.view(-1))), what + ': y0 changed'
            got = y.value().view(n, h, w, c)
            runs[mode] = got
            if integers:
                assert torch.equal(_bits(got), _bits(_bf16_of(ref))), what
            else:
                assert_bounded(got, ref, 13 * U32 * mag + lam, A_BF, 1.0, what=what, test=f'{ME}::test_sum_stats')
            if mode == 'no stats':
                assert stats.untouched(), what + ': stats = NULL, yet the rows were written'
                continue
            part = stats.value().view(torch.int32)
            assert not bool((part == 0x5A5B5C5D).any()), what + ': a partial row (or part of one) was never written'
            _check_stats(stats.value().double().view(2, rows, c), got, n, h, w, c, rows, tiled, what)
        assert torch.equal(_bits(runs['in place']), _bits(runs['out of place'])) and torch.equal(_bits(runs['in place']), _bits(runs['no stats']))


def _adj_args(ddp, outs, lows, n, h, w, c):
    a = [ddp, n, h, w, c]
    for j in range(3):
        a += [outs[j] and outs[j].ptr, lows[j][0], lows[j][1]] if j < len(lows) else [None, 1, 1]
    return a + [stream_ptr()]


@pytest.mark.parametrize('case', ADJ_CASES, ids=_case_id)
def test_bwd_multi(case):
    n, h, w, c, lows, tiled = case
    assert tiled_rule(n, h, w, c, lows, ADJ_GRID) == tiled
    lib = _C.lib()
    for integers in ((True, False) if _all_dyadic(h, w, lows) else (False,)):
        g = torch.Generator().manual_seed(h * 13 + c + len(lows) + 1000 * integers + 5)
        grad = _data((n, h, w, c), integers, g)
        ddst = gin(grad.cuda(), GUARD)
        outs = [gout(n * hs * ws * c, BF, GUARD) for hs, ws in lows]
        _C.check(lib.tok_bilinear_bwd_multi(*_adj_args(ddst.ptr, outs, lows, n, h, w, c)), 'tok_bilinear_bwd_multi')
        torch.cuda.synchronize()
        ddst.check('ddst')
        for (hs, ws), o in zip(lows, outs):
            what = f'{_case_id(case)} integers={integers} source {hs}x{ws}'
            o.check(what)
            got = o.value().view(n, hs, ws, c)
            assert not bool((_bits(got) == 0x5A5B).any()), what + ': an element was never written'
            ref = R.up64_T(grad, (hs, ws))
            if integers:
                assert torch.equal(_bits(got), _bits(_bf16_of(ref))), what
            else:
                taps = R.taps_T(hs, h) * R.taps_T(ws, w)
                assert_bounded(got, ref, (taps + 7) * U32 * R.up_T_mag(grad, (hs, ws)) + R.lam_term_T(grad, (hs, ws)), A_BF, 1.0,
                               what=what, test=f'{ME}::test_bwd_multi')


def test_bwd_multi_skips_null_sources():
    """a NULL source is skipped (every subset of the three present gives the same bits for those present and leaves the
    others' buffers alone); all three NULL returns OK and writes nothing"""
    n, h, w, c = 1, 32, 16, 72
    lows = _by_factor(h, w, (2, 4, 8))
    lib = _C.lib()
    grad = _data((n, h, w, c), True, torch.Generator().manual_seed(9))
    ddst = gin(grad.cuda(), GUARD)
    want = [_bits(_bf16_of(R.up64_T(grad, s))) for s in lows]
    for present in itertools.product((False, True), repeat=3):
        bufs = [gout(n * hs * ws * c, BF, GUARD) for hs, ws in lows]
        _C.check(lib.tok_bilinear_bwd_multi(*_adj_args(ddst.ptr, [b if p else None for b, p in zip(bufs, present)], lows, n, h, w, c)),
                 'tok_bilinear_bwd_multi')
        torch.cuda.synchronize()
        for (hs, ws), b, p, wnt in zip(lows, bufs, present, want):
            b.check(f'{present}')
            if p:
                assert torch.equal(_bits(b.value().view(n, hs, ws, c)), wnt), (present, hs, ws)
            else:
                assert b.untouched(), (present, hs, ws)


def _int_map(n, h, w, c, seed):
    """[n][h][w][c] bf16 integers in [-4, 4] made on the device, 256 rows at a time (no second copy of a 4 GB tensor)"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    out = torch.empty((n, h, w, c), dtype=BF, device='cuda')
    for lo in range(0, h, 256):
        out[:, lo:lo + 256] = torch.randint(-4, 5, (n, min(256, h - lo), w, c), generator=g, device='cuda', dtype=torch.int8)
    return out


BIG = (1, 2048, 2048, 520)       # n h w c > 2^31; 16384 tiles, inside the sum's grid limit of 65536
BANDS = ((0, 16), (1024, 1040), (2032, 2048))


def test_sum_stats_past_2_31_elements():
    """y [1][2048][2048][520] in place with the factor-8 source only: element offsets of the last rows lie past 2^31.  Integer
    data: bands of 16 rows at the top, the middle and the bottom are bit for bit the reference, evaluated on the device from
    slices; the partial rows of those tiles are the sums of the stored band.  (4.4 GB for y, 0.3 GB for the source and the
    partial rows; not shrunk.)"""
    n, h, w, c = BIG
    assert n * h * w * c > 2 ** 31 and tiled_rule(n, h, w, c, [(h // 8, w // 8)], SUM_GRID)
    lib = _C.lib()
    y = _int_map(n, h, w, c, 11)
    t8 = _int_map(n, h // 8, w // 8, c, 12)
    before = [y[:, lo:hi].clone() for lo, hi in BANDS]
    rows = lib.tok_bilinear_sum_stats_rows(n, h, w, c)
    assert rows == (h // 16) * (w // 16)
    stats = torch.full((2, rows, c), float('nan'), device='cuda')
    _C.check(lib.tok_bilinear_sum_stats(y.data_ptr(), t8.data_ptr(), h // 8, w // 8, None, 1, 1, None, 1, 1, n, h, w, c, y.data_ptr(),
                                        stats.data_ptr(), stream_ptr()), 'tok_bilinear_sum_stats')
    torch.cuda.synchronize()
    for (lo, hi), y0 in zip(BANDS, before):
        want = (y0.double() + R.up64(t8, (h, w), rows=(lo, hi))).to(BF)
        got = y[:, lo:hi]
        assert torch.equal(_bits(got), _bits(want)), (lo, hi)
        f = got.double().view(16, w // 16, 16, c)
        r0 = (lo // 16) * (w // 16)
        part = stats[:, r0:r0 + w // 16].double()
        assert_bounded(part[0], f.sum((0, 2)), f.abs().sum((0, 2)), 0.0, 11 * U32, f'tile sums of rows {lo}..{hi}')
        assert_bounded(part[1], (f * f).sum((0, 2)), (f * f).sum((0, 2)), 0.0, 11 * U32, f'tile squares of rows {lo}..{hi}')
    assert not bool(stats.isnan().any()), 'a partial row was never written'


def test_bwd_multi_past_2_31_elements():
    """ddst [1][2048][2048][520], the factor-8 source only.  Integer data: the two source rows under each 16-row band of ddst
    at the top, the middle and the bottom are bit for bit the reference transpose, evaluated on the device from the
    destination rows of their footprints."""
    n, h, w, c = BIG
    assert tiled_rule(n, h, w, c, [(h // 8, w // 8)], ADJ_GRID)
    lib = _C.lib()
    ddst = _int_map(n, h, w, c, 13)
    d8 = torch.full((n, h // 8, w // 8, c), float('nan'), dtype=BF, device='cuda')
    _C.check(lib.tok_bilinear_bwd_multi(ddst.data_ptr(), n, h, w, c, None, 1, 1, d8.data_ptr(), h // 8, w // 8, None, 1, 1, stream_ptr()),
             'tok_bilinear_bwd_multi')
    torch.cuda.synchronize()
    assert not bool(d8.isnan().any()), 'an element was never written'
    for lo, hi in BANDS:
        rows = (lo // 8, hi // 8)
        want = R.up64_T_rows(ddst, (h // 8, w // 8), rows).to(BF)
        assert torch.equal(_bits(d8[:, rows[0]:rows[1]]), _bits(want)), rows


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
_SUM_OK = dict(n=1, h=16, w=16, c=8, h1=8, w1=8, y0=True, y=True)
_SUM_BAD = [(dict(c=12), 'bad args'), (dict(c=0), 'bad args'), (dict(n=0), 'bad args'), (dict(h=0), 'bad args'), (dict(w=-16), 'bad args'),
            (dict(n=2 ** 19, h=64, w=64), 'bad args'), (dict(h1=0), 'term 1: bad size'), (dict(w1=-1), 'term 1: bad size'),
            (dict(y0=False), 'bad args'), (dict(y=False), 'bad args')]


@pytest.mark.parametrize('bad,msg', _SUM_BAD, ids=lambda v: ','.join(f'{k}={x}' for k, x in v.items()) if isinstance(v, dict) else None)
def test_sum_stats_refusals(bad, msg):
    """c % 8 != 0, non-positive extents, n h w >= 2^31, a present source with a non-positive size, a null y0 / y: the
    invalid-argument code, the message, nothing written"""
    lib = _C.lib()
    a = dict(_SUM_OK, **bad)
    y0, y, t1 = gout(16 * 16 * 16, BF, GUARD), gout(16 * 16 * 16, BF, GUARD), gout(8 * 8 * 16, BF, GUARD)
    stats = gout(2 * 16 * 16, F32, GUARD)
    rc = lib.tok_bilinear_sum_stats(y0.ptr if a['y0'] else None, t1.ptr, a['h1'], a['w1'], None, 1, 1, None, 1, 1, a['n'], a['h'], a['w'], a['c'],
                                    y.ptr if a['y'] else None, stats.ptr, stream_ptr())
    assert rc == ERR_INVALID and last_error() == 'tok_bilinear_sum_stats: ' + msg
    torch.cuda.synchronize()
    for buf in (y0, y, t1, stats):
        buf.check('refused call')
        assert buf.untouched()
    if min(a['n'], a['h'], a['w'], a['c']) <= 0 or a['c'] % 8:
        assert lib.tok_bilinear_sum_stats_rows(a['n'], a['h'], a['w'], a['c']) == ERR_INVALID


_ADJ_OK = dict(n=1, h=16, w=16, c=8, h1=8, w1=8, ddst=True)
_ADJ_BAD = [(dict(ddst=False), 'bad args'), (dict(n=0), 'bad args'), (dict(h=-16), 'bad args'), (dict(w=0), 'bad args'), (dict(c=0), 'bad args'),
            (dict(h1=0), 'source 1: bad size'), (dict(w1=-8), 'source 1: bad size')]


@pytest.mark.parametrize('bad,msg', _ADJ_BAD, ids=lambda v: ','.join(f'{k}={x}' for k, x in v.items()) if isinstance(v, dict) else None)
def test_bwd_multi_refusals(bad, msg):
    """a null ddst, non-positive extents, a present source with a non-positive size"""
    lib = _C.lib()
    a = dict(_ADJ_OK, **bad)
    ddst, d1, d2 = gout(16 * 16 * 16, BF, GUARD), gout(8 * 8 * 16, BF, GUARD), gout(4 * 4 * 16, BF, GUARD)
    # (the refused source comes first: the valid one behind it must not have been written by then either)
    rc = lib.tok_bilinear_bwd_multi(ddst.ptr if a['ddst'] else None, a['n'], a['h'], a['w'], a['c'], d1.ptr, a['h1'], a['w1'], d2.ptr, 4, 4,
                                    None, 1, 1, stream_ptr())
    assert rc == ERR_INVALID and last_error() == 'tok_bilinear_bwd_multi: ' + msg
    torch.cuda.synchronize()
    for buf in (ddst, d1, d2):
        buf.check('refused call')
        assert buf.untouched()
