"""The stochastic-depth BatchNorm trio of csrc/bn_droppath.hip (tok_bn_droppath_fwd / _bwd_reduce / _bwd_apply) element by element
against fp64 of the same bf16 inputs and fp32 parameters; reference and bounds are derived in tests/bn_droppath_ref.py.  Every
operand sits between guards (helpers.gin: NaN, helpers.gout: sentinels); every case is launched twice and must give the same bits.

Shapes (n, rows_per_sample, c), chosen so that blocks and grid-stride trips straddle sample boundaries:
  (1, 1, 8)               the smallest legal shape
  (3, 5, 16)              rpb = 128: one block holds all three samples
  (4, 49, 24)             rpb = 85, three blocks: a sample boundary inside each
  (7, 1, 2048)            layer 4 at 32 px: every row its own sample, rpb = 1
  (3, 100, 2176)          272 groups: a ragged second channel trip, the sample walk restarted per trip
  (5, 257, 8)             rpb = 256, six blocks: a sample one row longer than a block
  (2, 1024 * 128 + 3, 8)  past the 1024-block cap: a second trip of the row loop, the walk carries across the sample boundary
Per shape: small integers with dyadic scale / shift and s in {0, 1, 1.25, 2, 4} (out, mask, both partial sums, dy and dshortcut bit
for bit the fp64 values, rounded once); reals with s in {0, 1/0.9, 1/0.5} within the bounds, no element left out; s == 1 bit
for bit the plain trio tok_bn_act_fwd / tok_bn_bwd_reduce / tok_bn_bwd_apply; one sample dropped; all samples dropped; dshortcut
with = and += onto a prefill and aliasing dout; the forward without a mask.  The chain on the device's own intermediates at
(4, 49, 24), the completion event, and every refusal with the outputs untouched behind sentinels."""
import pytest
import torch

import bn_droppath_ref as D
import bn_ref as B
from helpers import BF, ERR_INVALID, F32, SENTINEL, U8, _INT_OF, gin, gout, last_error, unpack_bits
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
GUARD = 4096


def _written(g, what):
    g.check(what)
    assert int((g.view.view(_INT_OF[g.dtype]) == SENTINEL[g.dtype]).sum()) == 0, f'{what}: owned elements never written'
    if g.dtype != U8:
        assert bool(torch.isfinite(g.view.float()).all()), f'{what}: not finite'
    return g.value()


def _rows(m, c):
    got, want = _C.lib().tok_bn_bwd_rows(m, c), B.part_rows(m, c)
    assert got == want, f'tok_bn_bwd_rows({m}, {c}) = {got}, not {want}: is TOK_BN_BLOCKS set in the environment?'
    return want


class _Dev:
    """the inputs of one case on the device, each between NaN guards"""

    def __init__(self, d):
        self.big = {k: gin(d[k], GUARD) for k in ('y', 'shortcut', 'dout')}
        self.vec = {k: gin(d[k], 64) for k in ('scale', 'shift', 'mean', 'rstd', 'coef', 's')}

    def check(self):
        for k, g in list(self.big.items()) + list(self.vec.items()):
            g.check(k)


def _forward(dev, n, rps, c, with_mask=True):
    lib, st = _C.lib(), stream_ptr()
    m = n * rps
    v, b = dev.vec, dev.big
    out, mask = gout(m * c, BF, GUARD), gout(m * c // 8, U8, GUARD)
    _C.check(lib.tok_bn_droppath_fwd(b['y'].ptr, v['scale'].ptr, v['shift'].ptr, b['shortcut'].ptr, v['s'].ptr, rps, out.ptr,
                                     mask.ptr if with_mask else None, m, c, st), 'droppath_fwd')
    torch.cuda.synchronize()
    dev.check()
    mask.check('mask')
    if not with_mask:
        assert mask.untouched()
    return dict(out=_written(out, 'out').view(m, c), mask=mask.value() if with_mask else None, mask_dev=mask)


def _backward(dev, n, rps, c, mask_ptr, ds_mode, acc, ds0):
    """ds_mode: None, 'own' (a buffer of its own, prefilled with ds0 under acc) or 'alias' (dshortcut is dout)"""
    lib, st = _C.lib(), stream_ptr()
    m = n * rps
    rows = _rows(m, c)
    v, b = dev.vec, dev.big
    part = gout(2 * rows * c, F32, GUARD)
    _C.check(lib.tok_bn_droppath_bwd_reduce(b['dout'].ptr, b['y'].ptr, mask_ptr, v['s'].ptr, rps, v['mean'].ptr, v['rstd'].ptr, m, c,
                                            part.ptr, st), 'droppath_bwd_reduce')
    dy = gout(m * c, BF, GUARD)
    dout, ds = b['dout'], None
    if ds_mode == 'alias':
        dout = ds = gout(m * c, BF, GUARD, init=b['dout'].view)
    elif ds_mode == 'own':
        ds = gout(m * c, BF, GUARD, init=ds0.cuda() if acc else None)
    _C.check(lib.tok_bn_droppath_bwd_apply(dout.ptr, b['y'].ptr, mask_ptr, v['s'].ptr, rps, v['coef'].ptr, dy.ptr,
                                           ds.ptr if ds is not None else None, acc, m, c, st), 'droppath_bwd_apply')
    torch.cuda.synchronize()
    dev.check()
    return dict(part=_written(part, 'bwd partial').view(2, rows, c), dy=_written(dy, 'dy').view(m, c),
                ds=None if ds is None else _written(ds, 'dshortcut').view(m, c))


def _same(a, b, what):
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), f'{what}: {k} differs between two launches'


def _case(tag, n, rps, c, integer, mode, accs=(0, 1), alias=True):
    """forward and backward of one draw against fp64; returns (inputs, reference, device results) for the caller's own checks"""
    m = n * rps
    d = D.inputs(n, rps, c, integer, mode=mode)
    dev = _Dev(d)
    ref = D.DropRef(d)
    f = _forward(dev, n, rps, c)
    _same(f, _forward(dev, n, rps, c), 'forward')
    D.check_out(tag, ref, f['out'], integer)
    bits = unpack_bits(f['mask'], m, c)
    D.check_mask(f['out'], bits)
    if integer:
        assert torch.equal(bits, ref.pattern), 'mask bits differ from the fp64 pattern'
    assert torch.equal(_forward(dev, n, rps, c, with_mask=False)['out'], f['out']), 'out without a mask'
    # backward, alone: the mask is an input (the fp64 pattern)
    mk = gin(ref.mask_bytes, GUARD)
    res = {}
    for acc in accs:
        b = ref.bwd(ref.pattern, acc)
        if integer:
            D.assert_exact(d, b)
        r = _backward(dev, n, rps, c, mk.ptr, 'own', acc, d['ds0'])
        _same(r, _backward(dev, n, rps, c, mk.ptr, 'own', acc, d['ds0']), 'backward')
        D.check_sums(tag, r['part'].double().sum(1), b, m, c, integer)
        D.check_apply(f'{tag}_acc{acc}', b, r['dy'], r['ds'], acc, integer)
        res[acc] = (b, r)
    if alias:
        b, r = res[accs[0]]
        al = _backward(dev, n, rps, c, mk.ptr, 'alias', 0, None)       # in-place masking of the incoming gradient
        assert torch.equal(al['dy'], r['dy']) and torch.equal(al['part'], r['part'])
        D.check_apply(tag + '_alias', ref.bwd(ref.pattern, 0), al['dy'], al['ds'], 0, integer)
        none = _backward(dev, n, rps, c, mk.ptr, None, 0, None)        # no dshortcut at all
        assert torch.equal(none['dy'], r['dy'])
    mk.check('mask (input)')
    return d, dev, ref, f, res, mk


@pytest.mark.parametrize('n,rps,c', D.SHAPES)
def test_trio_vs_fp64(n, rps, c):
    big = n * rps > 100000
    for integer in (True, False):
        tag = f'bn_droppath_contract/{n}x{rps}x{c}_{"int" if integer else "real"}'
        _case(tag, n, rps, c, integer, 'mixed', accs=(1,) if big else (0, 1))


@pytest.mark.parametrize('n,rps,c', D.SHAPES)
def test_unit_scale_is_the_plain_trio_bit_for_bit(n, rps, c):
    lib, st = _C.lib(), stream_ptr()
    m = n * rps
    rows = _rows(m, c)
    d = D.inputs(n, rps, c, False, mode='ones')
    dev = _Dev(d)
    v, b = dev.vec, dev.big
    f = _forward(dev, n, rps, c)
    out, mask = gout(m * c, BF, GUARD), gout(m * c // 8, U8, GUARD)
    _C.check(lib.tok_bn_act_fwd(b['y'].ptr, v['scale'].ptr, v['shift'].ptr, b['shortcut'].ptr, 1, out.ptr, mask.ptr, m, c, st), 'act_fwd')
    part, dy = gout(2 * rows * c, F32, GUARD), gout(m * c, BF, GUARD)
    ds = gout(m * c, BF, GUARD, init=d['ds0'].cuda())
    _C.check(lib.tok_bn_bwd_reduce(b['dout'].ptr, b['y'].ptr, mask.ptr, v['scale'].ptr, v['shift'].ptr, v['mean'].ptr, v['rstd'].ptr, 1,
                                   m, c, part.ptr, st), 'bwd_reduce')
    _C.check(lib.tok_bn_bwd_apply(b['dout'].ptr, b['y'].ptr, mask.ptr, v['scale'].ptr, v['shift'].ptr, v['coef'].ptr, 1, dy.ptr, ds.ptr,
                                  1, m, c, st), 'bwd_apply')
    torch.cuda.synchronize()
    assert torch.equal(f['out'], _written(out, 'plain out').view(m, c)) and torch.equal(f['mask'], mask.value())
    r = _backward(dev, n, rps, c, f['mask_dev'].ptr, 'own', 1, d['ds0'])
    assert torch.equal(r['part'], _written(part, 'plain partial').view(2, rows, c))
    assert torch.equal(r['dy'], _written(dy, 'plain dy').view(m, c))
    assert torch.equal(r['ds'], _written(ds, 'plain dshortcut').view(m, c))


@pytest.mark.parametrize('n,rps,c', [s for s in D.SHAPES if s[0] > 1])
def test_one_dropped_sample(n, rps, c):
    """its out is exactly relu(shortcut), its dshortcut exactly dt, and its dy exactly c2 y + c3, which is not zero"""
    for integer in (True, False):
        tag = f'bn_droppath_contract/one_dropped_{n}x{rps}x{c}_{"int" if integer else "real"}'
        d, dev, ref, f, res, mk = _case(tag, n, rps, c, integer, 'one_dropped', accs=(0,), alias=False)
        i = n // 2
        rows = slice(i * rps, (i + 1) * rps)
        assert float(d['s'][i]) == 0.0 and float(d['s'].abs().sum()) > 0
        assert torch.equal(f['out'][rows], d['shortcut'][rows].float().clamp_min(0).to(BF)), 'out of the dropped sample is not relu(shortcut)'
        b, r = res[0]
        assert torch.equal(r['ds'][rows].double(), b['dt'][rows]), 'dshortcut of the dropped sample is not dt'
        want, mag = b['dy_dropped'][rows], b['m_dy_dropped'][rows]
        assert float(want.abs().max()) > 0
        if integer:
            B._eq(r['dy'][rows], D.bf_round(want), 'dy of the dropped sample')
        else:
            from helpers import A_BF, assert_bounded
            assert_bounded(r['dy'][rows], want, mag, A_BF, D.B_DY, 'dy of the dropped sample', tag)
        assert float(r['dy'][rows].float().abs().max()) > 0, 'the dropped sample received no batch-statistics terms'
        # the very same bits as a sample whose incoming gradient is zero: nothing but dz = 0 distinguishes a dropped sample
        d0 = dict(d, dout=d['dout'].clone())
        d0['dout'][rows] = 0
        r0 = _backward(_Dev(d0), n, rps, c, mk.ptr, 'own', 0, None)
        assert torch.equal(r0['dy'][rows], r['dy'][rows]) and torch.equal(r0['part'], r['part'])


@pytest.mark.parametrize('n,rps,c', D.SHAPES)
def test_all_samples_dropped(n, rps, c):
    d, dev, ref, f, res, mk = _case(f'bn_droppath_contract/zeros_{n}x{rps}x{c}', n, rps, c, False, 'zeros', accs=(0,), alias=False)
    b, r = res[0]
    assert bool((r['part'] == 0).all()), 'partial sums of a step with every sample dropped are not exactly 0'
    assert torch.equal(f['out'], d['shortcut'].float().clamp_min(0).to(BF))
    assert torch.equal(r['ds'].double(), b['dt'])


def test_chain_on_the_devices_own_intermediates():
    """tok_bn_stats -> tok_bn_finalize -> droppath_fwd -> droppath_bwd_reduce -> tok_bn_bwd_finalize -> droppath_bwd_apply"""
    lib, st = _C.lib(), stream_ptr()
    n, rps, c = 4, 49, 24
    m = n * rps
    rows = _rows(m, c)
    d = D.inputs(n, rps, c, False, seed=1)
    g = torch.Generator().manual_seed(11)
    gamma, beta = 1.0 + 0.3 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)
    runs = []
    for _ in range(2):
        dev = _Dev(d)
        ga, be = gin(gamma, 64), gin(beta, 64)
        stats = gout(2 * rows * c, F32, GUARD)
        _C.check(lib.tok_bn_stats(dev.big['y'].ptr, m, c, stats.ptr, st), 'stats')
        vec = {k: gout(c, F32, 64) for k in ('mean', 'rstd', 'scale', 'shift')}
        _C.check(lib.tok_bn_finalize(stats.ptr, rows, m, c, c, ga.ptr, be.ptr, None, None, None, B.MOMENTUM, B.EPS, vec['mean'].ptr,
                                     vec['rstd'].ptr, vec['scale'].ptr, vec['shift'].ptr, st), 'finalize')
        out, mask = gout(m * c, BF, GUARD), gout(m * c // 8, U8, GUARD)
        _C.check(lib.tok_bn_droppath_fwd(dev.big['y'].ptr, vec['scale'].ptr, vec['shift'].ptr, dev.big['shortcut'].ptr, dev.vec['s'].ptr,
                                         rps, out.ptr, mask.ptr, m, c, st), 'droppath_fwd')
        part = gout(2 * rows * c, F32, GUARD)
        _C.check(lib.tok_bn_droppath_bwd_reduce(dev.big['dout'].ptr, dev.big['y'].ptr, mask.ptr, dev.vec['s'].ptr, rps, vec['mean'].ptr,
                                                vec['rstd'].ptr, m, c, part.ptr, st), 'droppath_bwd_reduce')
        coef, dg, db = gout(3 * c, F32, 64), gout(c, F32, 64), gout(c, F32, 64)
        _C.check(lib.tok_bn_bwd_finalize(part.ptr, rows, m, c, c, ga.ptr, vec['mean'].ptr, vec['rstd'].ptr, dg.ptr, db.ptr, coef.ptr, 0, 0,
                                         st), 'bwd_finalize')
        dy, ds = gout(m * c, BF, GUARD), gout(m * c, BF, GUARD)
        _C.check(lib.tok_bn_droppath_bwd_apply(dev.big['dout'].ptr, dev.big['y'].ptr, mask.ptr, dev.vec['s'].ptr, rps, coef.ptr, dy.ptr,
                                               ds.ptr, 0, m, c, st), 'droppath_bwd_apply')
        torch.cuda.synchronize()
        dev.check()
        runs.append(dict(out=_written(out, 'out').view(m, c), dy=_written(dy, 'dy').view(m, c), ds=_written(ds, 'ds').view(m, c),
                         mask=mask.value(), dg=_written(dg, 'dgamma'), db=_written(db, 'dbeta')))
    _same(runs[0], runs[1], 'chain')
    r = runs[0]
    D.check_mask(r['out'], unpack_bits(r['mask'], m, c))
    ref = D.ChainRef(d, gamma, beta)
    ref.check('bn_droppath_contract/chain', r['out'], r['dy'], r['ds'])
    ag = D.autograd_fp64(d, gamma, beta)
    assert float((r['dg'].double() - ag['dgamma']).abs().max() / ag['dgamma'].abs().max()) < 1e-2
    assert float((r['db'].double() - ag['dbeta']).abs().max() / ag['dbeta'].abs().max()) < 1e-2


def test_bwd_apply_with_a_completion_event():
    """tok_next_launch_event(ev): the next tok_bn_droppath_bwd_apply signals ev as tok_bn_bwd_apply does; the launch after it
    carries none; a refused call uses the event up as well"""
    lib, st = _C.lib(), stream_ptr()
    n, rps, c = 2, 1024 * 128 + 3, 8
    m = n * rps
    d = D.inputs(n, rps, c, False)
    dev = _Dev(d)
    ref = D.DropRef(d)
    mk = gin(ref.mask_bytes, GUARD)
    plain = _backward(dev, n, rps, c, mk.ptr, 'own', 1, d['ds0'])
    v, b = dev.vec, dev.big
    ev = lib.tok_event_create()
    assert ev
    dy, ds = gout(m * c, BF, GUARD), gout(m * c, BF, GUARD, init=d['ds0'].cuda())
    side = torch.cuda.Stream()
    copy = torch.zeros(m * c, dtype=BF, device='cuda')
    torch.cuda.synchronize()
    assert lib.tok_next_launch_event(ev) == 0
    _C.check(lib.tok_bn_droppath_bwd_apply(b['dout'].ptr, b['y'].ptr, mk.ptr, v['s'].ptr, rps, v['coef'].ptr, dy.ptr, ds.ptr, 1, m, c,
                                           st), 'droppath_bwd_apply with an event')
    assert lib.tok_stream_wait_event(side.cuda_stream, ev) == 0, last_error()
    with torch.cuda.stream(side):
        copy.copy_(dy.view)
    side.synchronize()
    assert torch.equal(copy.cpu().view(m, c), plain['dy']), 'the side stream copied dy before the kernel had finished'
    torch.cuda.synchronize()
    assert torch.equal(_written(dy, 'dy').view(m, c), plain['dy']) and torch.equal(_written(ds, 'dshortcut').view(m, c), plain['ds'])
    _same(plain, _backward(dev, n, rps, c, mk.ptr, 'own', 1, d['ds0']), 'launch after the event')
    assert lib.tok_next_launch_event(ev) == 0
    assert lib.tok_bn_droppath_bwd_apply(b['dout'].ptr, b['y'].ptr, None, v['s'].ptr, rps, v['coef'].ptr, dy.ptr, None, 0, m, c,
                                         st) == ERR_INVALID
    _same(plain, _backward(dev, n, rps, c, mk.ptr, 'own', 1, d['ds0']), 'launch after a refused call that held the event')
    torch.cuda.synchronize()
    assert lib.tok_event_destroy(ev) == 0


def test_refusals_write_nothing():
    lib, st = _C.lib(), stream_ptr()
    n, rps, c = 3, 5, 16
    m = n * rps
    d = D.inputs(n, rps, c, False)
    dev = _Dev(d)
    v, b = dev.vec, dev.big
    mk = gin(D.DropRef(d).mask_bytes, GUARD)
    rows = _rows(m, c)
    outs = dict(out=gout(m * c, BF, GUARD), mask=gout(m * c // 8, U8, GUARD), part=gout(2 * rows * c, F32, GUARD),
                dy=gout(m * c, BF, GUARD), ds=gout(m * c, BF, GUARD))

    def fwd(y=b['y'].ptr, scale=v['scale'].ptr, shift=v['shift'].ptr, shortcut=b['shortcut'].ptr, s=v['s'].ptr, rps=rps,
            out=outs['out'].ptr, m=m, c=c):
        return lib.tok_bn_droppath_fwd(y, scale, shift, shortcut, s, rps, out, outs['mask'].ptr, m, c, st)

    def reduce(dout=b['dout'].ptr, y=b['y'].ptr, mask=mk.ptr, s=v['s'].ptr, rps=rps, m=m, c=c):
        return lib.tok_bn_droppath_bwd_reduce(dout, y, mask, s, rps, v['mean'].ptr, v['rstd'].ptr, m, c, outs['part'].ptr, st)

    def apply(dout=b['dout'].ptr, y=b['y'].ptr, mask=mk.ptr, s=v['s'].ptr, rps=rps, dy=outs['dy'].ptr, m=m, c=c):
        return lib.tok_bn_droppath_bwd_apply(dout, y, mask, s, rps, v['coef'].ptr, dy, outs['ds'].ptr, 0, m, c, st)

    sizes = [dict(c=12), dict(c=0), dict(m=0), dict(m=-m), dict(rps=0), dict(rps=-5), dict(rps=4), dict(rps=m + 1)]
    cases = [(fwd, 'tok_bn_droppath_fwd', sizes + [dict(s=None), dict(shortcut=None), dict(y=None), dict(out=None)]),
             (reduce, 'tok_bn_droppath_bwd_reduce', sizes + [dict(s=None), dict(mask=None), dict(y=None), dict(dout=None)]),
             (apply, 'tok_bn_droppath_bwd_apply', sizes + [dict(s=None), dict(mask=None), dict(y=None), dict(dout=None), dict(dy=None)])]
    for fn, name, bad in cases:
        for kw in bad:
            assert fn(**kw) == ERR_INVALID, (name, kw)
            assert name in last_error(), (name, kw, last_error())
    torch.cuda.synchronize()
    for k, g in outs.items():
        g.check(k)
        assert g.untouched(), f'{k}: written by a refused call'
    dev.check()
    assert fwd() == 0 and reduce() == 0 and apply() == 0, last_error()        # the same closures with nothing wrong do run
    torch.cuda.synchronize()
    for k, g in outs.items():
        _written(g, k)
