"""Kernel contract of csrc/pool.hip, element by element against tests/pool_ref.py (fp64 on the CPU from the bf16 inputs; that
module is held to ATen by tests/test_pool_ref.py and holds the table of bounds with their justification).

Every operand sits in a helpers.GuardedSpan: inputs between NaN guards, outputs filled with sentinels between sentinel guards
that are checked after the call.  Max and argmax results are compared bit for bit, integer-valued sums bit for bit, reals with
helpers.assert_bounded.  The cases that exist to reach a branch (a second grid-stride trip, trailing blocks without rows, idle
threads, the 64 KB LDS limit) assert from the launch arithmetic that they do.

Recorded err / bound above 0.5 (up to 0.996): every bf16 output.  A_BF = 2^-8 is the largest relative error of ONE
round-to-nearest to bf16 (half a unit in the last of 8 significant bits), and an exact kernel attains it whenever a result falls
half way between two bf16 values just above a power of two, which among 10^5 results always happens.  The bound cannot be
tighter without refusing a correctly rounded result; what is left for the accumulation is the k * U32 term, 2^-16 of the first.
The fp32 outputs (tok_colsum, tok_colsum_partial) carry no such term and stay below 0.07."""
import pytest
import torch

import pool_ref as R
from helpers import A_BF, BF, ERR_INVALID, F32, SENTINEL, U8, U32, assert_bounded, cdiv, gin, gout, last_error
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
G = 64                                   # guard elements on either side (GuardedSpan rounds up to 256 bytes)
I32 = torch.int32
MOD = 'test_pool_contract_gpu::'


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_bits(got, want64, what):
    """got (bf16, host) is bit for bit the bf16 of the fp64 reference (which must be representable: asserted)"""
    want = want64.to(BF)
    assert torch.equal(want.double().nan_to_num(nan=3.0), want64.nan_to_num(nan=3.0)), what + ': reference not representable'
    assert torch.equal(_bits(got), _bits(want.view(got.shape))), what


def _run(fn, *args):
    _C.check(getattr(_C.lib(), fn)(*args, stream_ptr()), fn)
    torch.cuda.synchronize()


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(v) * p for v, p in zip(key, (1, 131, 17, 7, 3, 1009, 31))) & 0x7fffffff)


def _reals(shape, g):
    return torch.randn(shape, generator=g).to(BF)


def _ints(shape, g, lim=4):
    return torch.randint(-lim, lim + 1, shape, generator=g).to(BF)


# ---- max-pool ------------------------------------------------------------------------------------------------------------------
def _maxpool_fwd_device(x):
    n, h, w, c = x.shape
    P, Q = R.pooled(h), R.pooled(w)
    xs = gin(x, G)
    y, am = gout(n * P * Q * c, BF, G), gout(n * P * Q * c, U8, G)
    _run('tok_maxpool3x3s2_fwd', xs.ptr, y.ptr, am.ptr, n, h, w, c)
    y.check('y'), am.check('argmax'), xs.check('x')
    return y.value().view(n, P, Q, c), am.value().view(n, P, Q, c)


@pytest.mark.parametrize('shape,family', [(s, f) for s in R.MAXPOOL_SHAPES for f in R.FAMILIES] + [(R.MAXPOOL_FWD_BIG, 'ties')],
                         ids=str)
def test_maxpool_forward_values_and_argmax_bit_for_bit(shape, family):
    n, h, w, c = shape
    if shape == R.MAXPOOL_FWD_BIG:
        assert n * R.pooled(h) * R.pooled(w) * c // 8 > R.CAP               # a second grid-stride trip
    x = R.maxpool_input(shape, family)
    best, tap = R.maxpool_fwd(x)
    y, am = _maxpool_fwd_device(x)
    assert torch.equal(am.long(), tap), f'{shape} {family}: argmax'
    if family == 'nan':
        assert torch.equal(y.isnan(), best.isnan()), 'NaN positions'
        fin = ~best.isnan()
        assert torch.equal(y.double()[fin], best[fin])
    else:
        _same_bits(y, best, f'{shape} {family}: values')


@pytest.mark.parametrize('shape', R.MAXPOOL_SHAPES + [R.MAXPOOL_BWD_BIG], ids=str)
def test_maxpool_backward_is_the_scatter(shape):
    n, h, w, c = shape
    P, Q = R.pooled(h), R.pooled(w)
    big = shape == R.MAXPOOL_BWD_BIG
    if big:
        assert n * h * w * c // 8 > R.CAP
    _, tap_dev = _maxpool_fwd_device(R.maxpool_input(shape, 'ties'))
    taps = [('device', tap_dev.long())]
    if h >= 3 and w >= 3 and not big:          # all four windows of the interior odd / odd pixel (1, 1) point at it
        hand = tap_dev.long().clone()
        for p in (0, 1):
            for q in (0, 1):
                hand[:, p, q] = (1 - (2 * p - 1)) * 3 + (1 - (2 * q - 1))
        count = R.maxpool_bwd(torch.ones(n, P, Q, c), hand, h, w)
        assert bool((count[:, 1, 1] == 4).all())                               # the 4-term sum
        taps.append(('hand', hand))
    for name, tap in taps:
        ams = gin(tap.to(U8), G)
        for integers in ((True,) if big else (True, False)):
            for accumulate in (0, 1):
                g = _gen(n, h, w, c, integers, accumulate)
                dy = (_ints if integers else _reals)((n, P, Q, c), g)
                prev = (_ints if integers else _reals)(shape, g)
                dys = gin(dy, G)
                dx = gout(n * h * w * c, BF, G, init=prev.cuda() if accumulate else None)
                _run('tok_maxpool3x3s2_bwd', dys.ptr, ams.ptr, dx.ptr, accumulate, n, h, w, c)
                what = f'{shape} argmax={name} integers={integers} accumulate={accumulate}'
                dx.check(what)
                got = dx.value().view(shape)
                ref = R.maxpool_bwd(dy, tap, h, w, prev if accumulate else None)
                if integers:                    # |sum| <= 4 * 4 + 4: exact
                    assert torch.equal(got.double(), ref), what
                else:
                    mag = R.maxpool_bwd(dy.abs(), tap, h, w, prev.abs() if accumulate else None)
                    assert_bounded(got, ref, mag, A_BF, 4 * U32, what=what, test=MOD + 'test_maxpool_backward_is_the_scatter')


# ---- avgpool2x2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', sorted({(s[1], s[2]) for s in R.AVGPOOL_SHAPES}), ids=str)
def test_avgpool2x2_forward_and_backward(hw):
    h, w = hw
    P, Q = R.pooled(h), R.pooled(w)
    for shape in [s for s in R.AVGPOOL_SHAPES if (s[1], s[2]) == hw]:
        n, _, _, c = shape
        for exact in (True, False):
            x = R.avg_exact_input(shape) if exact else _reals(shape, _gen(*shape, 1))
            xs, y = gin(x, G), gout(n * P * Q * c, BF, G)
            _run('tok_avgpool2x2_fwd', xs.ptr, y.ptr, n, h, w, c)
            y.check(f'y {shape}')
            got, ref = y.value().view(n, P, Q, c), R.avgpool_fwd(x)
            if exact:
                _same_bits(got, ref, f'forward {shape}')
            else:
                assert_bounded(got, ref, R.avgpool_fwd(x.abs()), A_BF, 5 * U32, what=f'forward {shape}',
                               test=MOD + 'test_avgpool2x2_forward_and_backward')
            for accumulate in (0, 1):
                g = _gen(*shape, 2, accumulate)
                dy = R.avg_exact_input((n, P, Q, c), 1) if exact else _reals((n, P, Q, c), g)
                prev = _ints(shape, g) if exact else _reals(shape, g)
                dys = gin(dy, G)
                dx = gout(n * h * w * c, BF, G, init=prev.cuda() if accumulate else None)
                _run('tok_avgpool2x2_bwd', dys.ptr, dx.ptr, accumulate, n, h, w, c)
                what = f'backward {shape} exact={exact} accumulate={accumulate}'
                dx.check(what)
                got = dx.value().view(shape)
                ref = R.avgpool_bwd(dy, h, w, prev if accumulate else None)
                if exact:                       # quotients of multiples of 4 by 1, 2, 4 plus integers |.| <= 4: exact
                    _same_bits(got, ref, what)
                else:
                    mag = R.avgpool_bwd(dy.abs(), h, w, prev.abs() if accumulate else None)
                    assert_bounded(got, ref, mag, A_BF, 3 * U32, what=what, test=MOD + 'test_avgpool2x2_forward_and_backward')


# ---- global average pool ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', R.GAP_SHAPES + [R.GAP_BWD_BIG], ids=str)
def test_gap_forward_and_backward(shape):
    n, hw, c = shape
    big = shape == R.GAP_BWD_BIG
    if big:
        assert n * hw * c // 8 > R.CAP
    else:
        x = _reals(shape, _gen(*shape, 1))
        xs, y = gin(x, G), gout(n * c, BF, G)
        _run('tok_gap_fwd', xs.ptr, y.ptr, n, hw, c)
        y.check(f'y {shape}')
        assert_bounded(y.value().view(n, c), R.gap_fwd(x), x.double().abs().mean(1), A_BF, (hw + 2) * U32,
                       what=f'forward {shape}', test=MOD + 'test_gap_forward_and_backward')
    for accumulate in (0, 1):
        g = _gen(*shape, 2, accumulate)
        dy, prev = _reals((n, c), g), _reals(shape, g)
        dys = gin(dy, G)
        dx = gout(n * hw * c, BF, G, init=prev.cuda() if accumulate else None)
        _run('tok_gap_bwd', dys.ptr, dx.ptr, accumulate, n, hw, c)
        what = f'backward {shape} accumulate={accumulate}'
        dx.check(what)
        ref = R.gap_bwd(dy, hw, prev if accumulate else None)
        mag = R.gap_bwd(dy.abs(), hw, prev.abs() if accumulate else None)
        assert_bounded(dx.value().view(shape), ref, mag, A_BF, 3 * U32, what=what, test=MOD + 'test_gap_forward_and_backward')


# ---- global max / avgmax / catavgmax ---------------------------------------------------------------------------------------------
def _global_fwd_device(x, mode, ldy):
    n, hw, c = x.shape
    xs = gin(x, G)
    y, am = gout(n * ldy, BF, G), gout(n * c, I32, G)
    _run('tok_global_pool_fwd', xs.ptr, y.ptr, am.ptr, n, hw, c, ldy, mode)
    y.check('y'), am.check('argmax')
    return y.value().view(n, ldy), am.value().view(n, c)


@pytest.mark.parametrize('family', R.FAMILIES + ('exact',))
@pytest.mark.parametrize('shape', R.GAP_SHAPES, ids=str)
def test_global_pool_forward(shape, family):
    n, hw, c = shape
    x = R.avgmax_exact_input(n, hw, c) if family == 'exact' else R.global_input(n, hw, c, family)
    mx, am = R.global_max(x)
    avg, absmean = R.gap_fwd(x), x.double().abs().mean(1)
    ok = torch.isfinite(avg)                 # ('neginf': the average of the -inf channel is -inf, 'nan': NaN, compared as such)
    test = MOD + 'test_global_pool_forward'
    for mode, ldy in ((1, c), (2, c), (3, 2 * c), (3, 2 * c + 8)):
        y, amd = _global_fwd_device(x, mode, ldy)
        what = f'{shape} {family} mode={mode} ldy={ldy}'
        assert torch.equal(amd.long(), am), what + ': argmax'
        used = 2 * c if mode == 3 else c
        assert bool((_bits(y[:, used:]) == SENTINEL[BF]).all()), what + ': pad columns written'
        ymax = y[:, c:2 * c] if mode == 3 else y
        if mode in (1, 3):                       # bit for bit; NaN by position (the payload is not part of the contract)
            assert torch.equal(ymax.isnan(), mx.isnan()), what
            assert torch.equal(ymax.double().nan_to_num(nan=3.0), mx.nan_to_num(nan=3.0)), what + ': max'
        if mode == 3:
            got = y[:, :c]
            assert torch.equal(got.double()[~ok].nan_to_num(nan=3.0), avg[~ok].nan_to_num(nan=3.0)), what
            if family == 'exact':
                _same_bits(got, avg, what + ': avg')
            else:
                assert_bounded(torch.where(ok, got.double(), 0.0), torch.where(ok, avg, 0.0), torch.where(ok, absmean, 0.0), A_BF,
                               (hw + 2) * U32, what=what + ' avg', test=test)
        if mode == 2:
            ref = R.avgmax_ref(x)
            fin = torch.isfinite(ref)
            assert torch.equal(y.double()[~fin].nan_to_num(nan=3.0), ref[~fin].nan_to_num(nan=3.0)), what
            if family == 'exact':
                _same_bits(y, ref, what + ': avgmax')
            else:
                a, rest = R.avgmax_bound(x)
                assert_bounded(torch.where(fin, y.double(), 0.0), torch.where(fin, ref, 0.0), torch.where(fin, rest, 0.0), a, 1.0,
                               what=what + ' avgmax', test=test)


@pytest.mark.parametrize('shape', R.GAP_SHAPES + [R.GAP_BWD_BIG], ids=str)
def test_global_pool_backward(shape):
    n, hw, c = shape
    big = shape == R.GAP_BWD_BIG
    if big:
        assert n * hw * c // 8 > R.CAP
    x = R.global_input(n, hw, c, 'ties')
    _, am = R.global_max(x)                       # ties: only pixel argmax (the first maximum) receives the max gradient
    assert hw == 1 or bool(((x.double() == x.double().amax(1, keepdim=True)).sum(1) > 1).any())
    ams = gin(am.to(I32), G)
    for mode, ldy in (((3, 2 * c + 8),) if big else ((1, c), (2, c), (3, 2 * c), (3, 2 * c + 8))):
        for accumulate in (0, 1):
            g = _gen(*shape, mode, ldy, accumulate)
            dy, prev = _reals((n, ldy), g), _reals(shape, g)
            used = 2 * c if mode == 3 else c
            dy[:, used:] = float('nan')                                        # pad columns of dy are not the kernel's
            dys = gin(dy, G)
            dx = gout(n * hw * c, BF, G, init=prev.cuda() if accumulate else None)
            _run('tok_global_pool_bwd', dys.ptr, ams.ptr, dx.ptr, accumulate, n, hw, c, ldy, mode)
            what = f'{shape} mode={mode} ldy={ldy} accumulate={accumulate}'
            dx.check(what)
            ref, mag = R.global_pool_bwd(dy, am, hw, mode, prev if accumulate else None)
            assert_bounded(dx.value().view(shape), ref, mag, A_BF, 4 * U32, what=what, test=MOD + 'test_global_pool_backward')


# ---- column sums -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', R.COLSUM_SHAPES, ids=str)
def test_colsum(shape):
    m, n_pad, n_real = shape
    for integers in (True, False):
        for accumulate in (0, 1):
            g = _gen(*shape, integers, accumulate)
            x = (_ints if integers else _reals)((m, n_pad), g)
            prev = torch.randint(-8, 9, (n_pad,), generator=g).float() if integers else torch.randn(n_pad, generator=g)
            xs = gin(x, G)
            out = gout(n_pad, F32, G)
            if accumulate:
                out.view[:n_real].copy_(prev[:n_real])
            _run('tok_colsum', xs.ptr, m, n_pad, n_real, out.ptr, accumulate)
            what = f'{shape} integers={integers} accumulate={accumulate}'
            out.check(what)
            got = out.value()
            assert bool((got[n_real:].view(I32) == SENTINEL[F32]).all()), what + ': a column at or past n_real written'
            ref = x.double().sum(0) + (prev.double() if accumulate else 0)
            if integers:                         # |sum| <= 4 m + 8 < 2^24: exact in every order
                assert torch.equal(got[:n_real].double(), ref[:n_real]), what
            else:
                mag = x.double().abs().sum(0) + (prev.double().abs() if accumulate else 0)
                assert_bounded(got[:n_real], ref[:n_real], mag[:n_real], 0.0, (cdiv(m, 256) + 9) * U32, what=what,
                               test=MOD + 'test_colsum')


@pytest.mark.parametrize('m,n_pad', [(m, p) for p in R.PARTIAL_NPAD for m in R.PARTIAL_M] + [R.PARTIAL_TALL], ids=str)
def test_colsum_partial(m, n_pad):
    lib = _C.lib()
    g_rows, chunk = R.partial_rows(m)
    assert lib.tok_colsum_partial_rows(m, n_pad) == g_rows
    cgs, cgt, rpb, idle, lds = R.partial_launch(n_pad)
    assert lds <= 64 * 1024
    assert {8: rpb == 256, 288: (cgs, rpb, idle) == (36, 7, 4), 2048: rpb == 1, 3072: cgs > cgt,
            16384: lds == 64 * 1024}[n_pad]                                   # the branch this n_pad is here for
    if (m, n_pad) == R.PARTIAL_TALL:
        assert (g_rows - 3) * chunk >= m                                      # the last three blocks own no row
    for integers in (True, False):
        x = (_ints if integers else _reals)((m, n_pad), _gen(m, n_pad, integers))
        xs = gin(x, G)
        part = gout(g_rows * n_pad, F32, G)
        _run('tok_colsum_partial', xs.ptr, m, n_pad, part.ptr)
        what = f'm={m} n_pad={n_pad} integers={integers}'
        part.check(what)
        got = part.value().view(g_rows, n_pad)
        assert not bool((got.view(I32) == SENTINEL[F32]).any()), what + ': a partial element was not written'
        ref, mag = R.colsum_partial(x, g_rows, chunk)
        if integers:
            assert torch.equal(got.double(), ref), what
            assert torch.equal(got.double().sum(0), x.double().sum(0)), what
        else:
            assert_bounded(got, ref, mag, 0.0, chunk * U32, what=what, test=MOD + 'test_colsum_partial')
    if (m, n_pad) == R.PARTIAL_TALL:
        assert bool((got[-3:].view(I32) == 0).all()), 'blocks without rows must write +0'


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """every TOK_CHECK_ARG of pool.hip: the invalid-argument code, the function named in tok_last_error, nothing written"""
    lib, st = _C.lib(), stream_ptr()
    src = gin(torch.zeros(4096, dtype=BF), G)
    out, out2 = gout(4096, BF, G), gout(4096, F32, G)
    i, o, f = src.ptr, out.ptr, out2.ptr
    ok4 = dict(n=1, h=4, w=4, c=8)

    def dims(**bad):
        d = dict(ok4, **bad)
        return d['n'], d['h'], d['w'], d['c']
    bad_dims = [dict(n=0), dict(h=0), dict(w=-1), dict(c=0), dict(c=12)]
    calls = []
    for b in bad_dims:
        calls += [('tok_maxpool3x3s2_fwd', (i, o, f, *dims(**b), st)), ('tok_maxpool3x3s2_bwd', (i, i, o, 0, *dims(**b), st)),
                  ('tok_avgpool2x2_fwd', (i, o, *dims(**b), st)), ('tok_avgpool2x2_bwd', (i, o, 0, *dims(**b), st))]
    calls += [('tok_maxpool3x3s2_fwd', (None, o, f, *dims(), st)), ('tok_maxpool3x3s2_fwd', (i, None, f, *dims(), st)),
              ('tok_maxpool3x3s2_fwd', (i, o, None, *dims(), st)), ('tok_maxpool3x3s2_bwd', (None, i, o, 0, *dims(), st)),
              ('tok_maxpool3x3s2_bwd', (i, None, o, 0, *dims(), st)), ('tok_maxpool3x3s2_bwd', (i, i, None, 0, *dims(), st)),
              ('tok_avgpool2x2_fwd', (None, o, *dims(), st)), ('tok_avgpool2x2_fwd', (i, None, *dims(), st)),
              ('tok_avgpool2x2_bwd', (None, o, 0, *dims(), st)), ('tok_avgpool2x2_bwd', (i, None, 0, *dims(), st))]
    for n, hw, c in ((0, 4, 8), (1, 0, 8), (1, 4, 0), (1, 4, 12)):
        calls += [('tok_gap_fwd', (i, o, n, hw, c, st)), ('tok_gap_bwd', (i, o, 0, n, hw, c, st)),
                  ('tok_global_pool_fwd', (i, o, f, n, hw, c, 16, 1, st)), ('tok_global_pool_bwd', (i, i, o, 0, n, hw, c, 16, 1, st))]
    calls += [('tok_gap_fwd', (None, o, 1, 4, 8, st)), ('tok_gap_fwd', (i, None, 1, 4, 8, st)),
              ('tok_gap_bwd', (None, o, 0, 1, 4, 8, st)), ('tok_gap_bwd', (i, None, 0, 1, 4, 8, st)),
              ('tok_global_pool_fwd', (None, o, f, 1, 4, 8, 8, 1, st)), ('tok_global_pool_fwd', (i, None, f, 1, 4, 8, 8, 1, st)),
              ('tok_global_pool_fwd', (i, o, None, 1, 4, 8, 8, 1, st)), ('tok_global_pool_bwd', (None, i, o, 0, 1, 4, 8, 8, 1, st)),
              ('tok_global_pool_bwd', (i, None, o, 0, 1, 4, 8, 8, 1, st)), ('tok_global_pool_bwd', (i, i, None, 0, 1, 4, 8, 8, 1, st))]
    for mode, ldy in ((0, 16), (4, 16), (1, 0), (2, 7), (3, 8), (3, 15), (1, 12), (3, 20)):      # mode, ldy < c / 2c, ldy % 8
        calls += [('tok_global_pool_fwd', (i, o, f, 1, 4, 8, ldy, mode, st)),
                  ('tok_global_pool_bwd', (i, i, o, 0, 1, 4, 8, ldy, mode, st))]
    for m, n_pad, n_real in ((0, 8, 8), (4, 0, 0), (4, 12, 8), (4, 8, 9), (4, 8, 0), (4, 8, -1)):
        calls.append(('tok_colsum', (i, m, n_pad, n_real, f, 0, st)))
    calls += [('tok_colsum', (None, 4, 8, 8, f, 0, st)), ('tok_colsum', (i, 4, 8, 8, None, 0, st))]
    for m, n_pad in ((0, 8), (4, 0), (4, 12), (4, 16392)):
        calls.append(('tok_colsum_partial', (i, m, n_pad, f, st)))
    calls += [('tok_colsum_partial', (None, 4, 8, f, st)), ('tok_colsum_partial', (i, 4, 8, None, st))]
    for fn, args in calls:
        rc = getattr(lib, fn)(*args)
        assert rc == ERR_INVALID and fn + ':' in last_error(), (fn, args[:-1], rc, last_error())
    torch.cuda.synchronize()
    for buf in (out, out2):
        buf.check('refused call')
        assert buf.untouched()
    src.check('refused call')
