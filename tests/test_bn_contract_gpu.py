"""The training BatchNorm chain and the fused stem of csrc/bn.hip element by element against fp64 of the same bf16 inputs and
fp32 parameters; references and bounds are derived in tests/bn_ref.py.  Every kernel runs twice: on small integers and dyadic
parameters, where the result must be the fp64 one bit for bit (coverage, ownership, indexing), and on random reals within the
rounding bounds.  Every operand sits between guards (helpers.gin: NaN, helpers.gout: sentinels); each case is launched twice
and must give the same bits.

Streaming kernels (tok_bn_stats, tok_bn_act_fwd[_colsum], tok_bn_bwd_reduce, tok_bn_bwd_apply), (m, c):
  (1, 8)              the smallest legal shape
  (37, 16)            two groups, rpb = 128, one partly filled block
  (171, 24)           3 groups, rpb = 85: one idle lane, two blocks and one row
  (98, 72)            rpb = 28: four idle lanes
  (777, 48)           rpb = 42, 19 blocks, the last one ragged
  (300, 2040)         255 groups, rpb = 1, one idle lane
  (300, 2048)         256 groups: the widest single pass
  (300, 2176)         272 groups: the channel-group loop with a ragged second trip (16 of 256 lanes live); tok_bn_act_fwd_colsum
                      refuses it and writes nothing
  (1027, 2048)        1024 blocks of one row, then three rows in a second trip of the row loop
  (70001, 8)          274 blocks of 256 rows, the last with 113
  (1024 * 256 + 257, 8)   over the 1024-block cap at rpb = 256: a second trip of 257 rows
with relu 0 / 1, shortcut or none, the mask given or NULL (no shortcut: bit-equal to the masked path), dshortcut = / += onto a
prefill and aliasing dout, and one tok_bn_bwd_apply carrying a completion event.
Finalize kernels (tok_bn_finalize, tok_bn_bwd_finalize) on rows the test writes: c in {8, 48, 264} (4 channels a block, 64 row
lanes) with rows on both sides of 64, 4 x 64, 8 x 64 and 16 x 64, c in {512, 520, 2048} (16 channels, 16 row lanes; 520 leaves
half a block) likewise around 16, 64, 128; a mean-64 channel, a constant channel, count = 1, no running statistics, c_real < c,
accumulate, NULL dgamma / dbeta, the dz y form.  The chain on the device's own intermediates at (777, 48) and (1027, 2048).
Fused stem (n, h, w, c): (1, 1, 1, 8), (1, 2, 3, 8), (2, 7, 9, 16), (3, 8, 8, 64) (even sizes: the last row and column belong to
one window only), (1, 15, 17, 8), (3, 57, 61, 256) (10431 rows at rpb = 8: a second trip of the row loop, the incremental
(n, h, w) stepping carries in all three digits)."""
import pytest
import torch

import bn_ref as R
from helpers import BF, ERR_INVALID, F32, SENTINEL, U8, _INT_OF, gin, gout, last_error, unpack_bits
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
GUARD = 4096          # elements: more than one row of the widest shape and any channel group
CONFIGS = [(1, 1, 1, 1), (1, 0, 1, 0), (1, 0, 0, 0), (0, 0, 0, 0), (0, 1, 0, 1)]        # relu, shortcut, mask given, ds_acc


def _written(g, what, nan_ok=False):
    """guards intact, every owned element written, nothing but finite values"""
    g.check(what)
    assert int((g.view.view(_INT_OF[g.dtype]) == SENTINEL[g.dtype]).sum()) == 0, f'{what}: owned elements never written'
    if g.dtype != U8 and not nan_ok:
        assert bool(torch.isfinite(g.view.float()).all()), f'{what}: not finite'
    return g.value()


def _rows(m, c):
    lib = _C.lib()
    want = R.part_rows(m, c)
    for fn in ('tok_bn_bwd_rows', 'tok_bn_stats_rows', 'tok_bn_act_fwd_colsum_rows'):
        got = getattr(lib, fn)(m, c)
        assert got == want, f'{fn}({m}, {c}) = {got}, not min(ceil(m / rpb), 1024) = {want}: is TOK_BN_BLOCKS set in the environment?'
    return want


class _Dev:
    """the inputs of one (m, c) on the device, each between NaN guards"""

    def __init__(self, d):
        self.big = {k: gin(d[k], GUARD) for k in ('y', 'shortcut', 'dout')}
        self.vec = {k: gin(d[k], 64) for k in ('scale', 'shift', 'mean', 'rstd', 'coef')}

    def check(self):
        for k, g in list(self.big.items()) + list(self.vec.items()):
            g.check(k)


def _forward(dev, m, c, relu, with_sc, rows):
    lib, st = _C.lib(), stream_ptr()
    v, b = dev.vec, dev.big
    sc = b['shortcut'].ptr if with_sc else None
    out, mask = gout(m * c, BF, GUARD), gout(m * c // 8, U8, GUARD)
    _C.check(lib.tok_bn_act_fwd(b['y'].ptr, v['scale'].ptr, v['shift'].ptr, sc, relu, out.ptr, mask.ptr, m, c, st), 'act_fwd')
    out1 = gout(m * c, BF, GUARD)
    _C.check(lib.tok_bn_act_fwd(b['y'].ptr, v['scale'].ptr, v['shift'].ptr, sc, relu, out1.ptr, None, m, c, st), 'act_fwd, no mask')
    out2, mask2, part = gout(m * c, BF, GUARD), gout(m * c // 8, U8, GUARD), gout(rows * c, F32, GUARD)
    rc = lib.tok_bn_act_fwd_colsum(b['y'].ptr, v['scale'].ptr, v['shift'].ptr, sc, relu, out2.ptr, mask2.ptr, m, c, part.ptr, st)
    torch.cuda.synchronize()
    dev.check()
    r = dict(out=_written(out, 'out'), mask=mask.value(), mask_dev=mask)
    mask.check('mask')
    assert torch.equal(_written(out1, 'out without a mask'), r['out'])
    if c > 2048:
        assert rc == ERR_INVALID and 'tok_bn_act_fwd_colsum' in last_error()
        assert out2.untouched() and mask2.untouched() and part.untouched()
        for g in (out2, mask2, part):
            g.check('refused colsum')
    else:
        assert rc == 0, last_error()
        mask2.check('colsum mask')
        assert torch.equal(_written(out2, 'colsum out'), r['out']) and torch.equal(mask2.value(), r['mask'])
        r['colsum'] = _written(part, 'colsum partial').view(rows, c)
    return r


def _backward(dev, m, c, relu, mask_ptr, ds_mode, acc, ds0, rows):
    """ds_mode: None, 'own' (a buffer of its own, prefilled with ds0 under acc) or 'alias' (dshortcut is dout)"""
    lib, st = _C.lib(), stream_ptr()
    v, b = dev.vec, dev.big
    part = gout(2 * rows * c, F32, GUARD)
    _C.check(lib.tok_bn_bwd_reduce(b['dout'].ptr, b['y'].ptr, mask_ptr, v['scale'].ptr, v['shift'].ptr, v['mean'].ptr, v['rstd'].ptr,
                                   relu, m, c, part.ptr, st), 'bwd_reduce')
    dy = gout(m * c, BF, GUARD)
    dout, ds = b['dout'], None
    if ds_mode == 'alias':
        dout = ds = gout(m * c, BF, GUARD, init=b['dout'].view)
    elif ds_mode == 'own':
        ds = gout(m * c, BF, GUARD, init=ds0.cuda() if acc else None)
    _C.check(lib.tok_bn_bwd_apply(dout.ptr, b['y'].ptr, mask_ptr, v['scale'].ptr, v['shift'].ptr, v['coef'].ptr, relu, dy.ptr,
                                  ds.ptr if ds is not None else None, acc, m, c, st), 'bwd_apply')
    torch.cuda.synchronize()
    dev.check()
    return dict(part=_written(part, 'bwd partial').view(2, rows, c), dy=_written(dy, 'dy').view(m, c),
                ds=None if ds is None else _written(ds, 'dshortcut').view(m, c))


def _same(a, b, what):
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), f'{what}: {k} differs between two launches'


@pytest.mark.parametrize('m,c', R.STREAM_SHAPES)
def test_streaming_kernels_vs_fp64(m, c):
    lib, st = _C.lib(), stream_ptr()
    rows = _rows(m, c)
    n = R.n_sum(m, c)
    configs = CONFIGS if m < 70000 else CONFIGS[:1] + CONFIGS[2:3]
    for integer in (True, False):
        tag = f'bn_contract/stream_{m}x{c}_{"int" if integer else "real"}'
        d = R.stream_inputs(m, c, integer)
        dev = _Dev(d)
        stats = []
        for _ in range(2):
            g = gout(2 * rows * c, F32, GUARD)
            _C.check(lib.tok_bn_stats(dev.big['y'].ptr, m, c, g.ptr, st), 'stats')
            torch.cuda.synchronize()
            stats.append(_written(g, 'stats').view(2, rows, c))
        assert torch.equal(stats[0], stats[1])
        for relu, with_sc, use_mask, acc in configs:
            ref = R.StreamRef(d, relu, with_sc)
            b = ref.bwd(use_mask, acc)
            if integer:
                R.assert_exact_sums(ref, b)
            t = f'{tag}_relu{relu}_sc{with_sc}_mask{use_mask}'
            f = _forward(dev, m, c, relu, with_sc, rows)
            _same(f, _forward(dev, m, c, relu, with_sc, rows), 'forward')
            out = f['out'].view(m, c)
            R.check_out(t, ref, out, integer)
            bits = unpack_bits(f['mask'], m, c)
            R.check_mask(ref, out, bits)
            if integer:
                assert torch.equal(bits, ref.pattern if relu else ref.out > 0)
            if 'colsum' in f:
                R.check_colsum(t, out, f['colsum'].double().sum(0), m, c, integer, ref)
            R.check_sums(t, 'stats', stats[0].double().sum(1), ref.y2, ref.m_y2, torch.zeros(2, c), n, integer)
            # backward, alone: the mask is an input (the fp64 pattern) or NULL
            mk = gin(ref.mask_bytes, GUARD) if use_mask else None
            ds_mode = None if (relu and not use_mask) else 'own'
            r = _backward(dev, m, c, relu, mk.ptr if mk else None, ds_mode, acc, d['ds0'], rows)
            _same(r, _backward(dev, m, c, relu, mk.ptr if mk else None, ds_mode, acc, d['ds0'], rows), 'backward')
            if mk:
                mk.check('mask (input)')
            R.check_sums(t, 'bwd_reduce', r['part'].double().sum(1), b['sums'], b['m_sums'], b['x_sums'], n, integer)
            R.check_apply(t, b, r['dy'], r['ds'], acc, integer)
            if relu and with_sc:
                # dshortcut aliasing dout (in-place masking of the incoming gradient), ds_acc = 0
                al = _backward(dev, m, c, relu, mk.ptr, 'alias', 0, None, rows)
                assert torch.equal(al['dy'], r['dy']) and torch.equal(al['part'], r['part'])
                R.check_apply(t + '_alias', ref.bwd(True, 0), al['dy'], al['ds'], 0, integer)
            if relu and not with_sc and not use_mask:
                # mask == NULL recomputes the pattern: bit for bit the masked path on the forward's own mask
                fm = _backward(dev, m, c, relu, f['mask_dev'].ptr, None, 0, None, rows)
                assert torch.equal(fm['dy'], r['dy']) and torch.equal(fm['part'], r['part'])


def test_bwd_apply_with_a_completion_event():
    """tok_next_launch_event(ev): the next tok_bn_bwd_apply signals ev when the kernel is done.  The same bits as a plain launch; a
    side stream that waits for ev and copies dy sees the complete tensor; the following launch carries no event."""
    lib, st = _C.lib(), stream_ptr()
    m, c = 1024 * 256 + 257, 8
    rows = _rows(m, c)
    d = R.stream_inputs(m, c, False)
    dev = _Dev(d)
    ref = R.StreamRef(d, 1, 1)
    mk = gin(ref.mask_bytes, GUARD)
    plain = _backward(dev, m, c, 1, mk.ptr, 'own', 1, d['ds0'], rows)
    v, b = dev.vec, dev.big
    ev = lib.tok_event_create()
    assert ev
    dy, ds = gout(m * c, BF, GUARD), gout(m * c, BF, GUARD, init=d['ds0'].cuda())
    side = torch.cuda.Stream()
    copy = torch.zeros(m * c, dtype=BF, device='cuda')
    torch.cuda.synchronize()
    assert lib.tok_next_launch_event(ev) == 0
    _C.check(lib.tok_bn_bwd_apply(b['dout'].ptr, b['y'].ptr, mk.ptr, v['scale'].ptr, v['shift'].ptr, v['coef'].ptr, 1, dy.ptr, ds.ptr, 1,
                                  m, c, st), 'bwd_apply with an event')
    assert lib.tok_stream_wait_event(side.cuda_stream, ev) == 0, last_error()
    with torch.cuda.stream(side):
        copy.copy_(dy.view)
    side.synchronize()
    assert torch.equal(copy.cpu().view(m, c), plain['dy']), 'the side stream copied dy before the kernel had finished'
    torch.cuda.synchronize()
    assert torch.equal(_written(dy, 'dy').view(m, c), plain['dy']) and torch.equal(_written(ds, 'dshortcut').view(m, c), plain['ds'])
    after = _backward(dev, m, c, 1, mk.ptr, 'own', 1, d['ds0'], rows)          # a plain launch again: the event is used up
    _same(plain, after, 'launch after the event')
    assert lib.tok_event_destroy(ev) == 0
    assert lib.tok_stream_wait_event(side.cuda_stream, None) == ERR_INVALID


# ---- finalize kernels ------------------------------------------------------------------------------------------------------
def _finalize(p, c, c_real=None, count=None, running=True):
    lib, st = _C.lib(), stream_ptr()
    cr = c if c_real is None else c_real
    rows = p['stats'].shape[1]
    sg = gin(p['stats'], GUARD)
    ga, be = gin(p['gamma'][:cr], 64), gin(p['beta'][:cr], 64)
    rm, rv = gout(cr, F32, 64, init=p['rm'][:cr].cuda()), gout(cr, F32, 64, init=p['rv'][:cr].cuda())
    nbt = torch.tensor([41], dtype=torch.int64, device='cuda')
    outs = [gout(c, F32, 64) for _ in range(4)]
    _C.check(lib.tok_bn_finalize(sg.ptr, rows, p['count'] if count is None else count, c, cr, ga.ptr, be.ptr, rm.ptr if running else None,
                                 rv.ptr if running else None, nbt.data_ptr(), R.MOMENTUM, R.EPS, *(o.ptr for o in outs), st), 'finalize')
    torch.cuda.synchronize()
    for g, what in ((sg, 'stats'), (ga, 'gamma'), (be, 'beta')):
        g.check(what)
    assert int(nbt) == 42, 'num_batches_tracked is incremented exactly once'
    res = [_written(o, w) for o, w in zip(outs, ('mean', 'rstd', 'scale', 'shift'))]
    if running:
        res += [_written(rm, 'running_mean'), _written(rv, 'running_var')]
    else:
        for g, src in ((rm, p['rm']), (rv, p['rv'])):
            g.check('running')
            assert torch.equal(g.value(), src[:cr]), 'running statistics written although NULL was passed'
    return res


def _bwd_finalize(q, c, dzy, acc, c_real=None, grads=True):
    lib, st = _C.lib(), stream_ptr()
    cr = c if c_real is None else c_real
    rows = q['part'].shape[1]
    pg, ga = gin(q['part'], GUARD), gin(q['gamma'][:cr], 64)
    mu, rs = gin(q['mean'], 64), gin(q['rstd'], 64)
    dg, db = (gout(cr, F32, 64, init=q['pre'][i][:cr].cuda() if acc else None) for i in (0, 1))
    coef = gout(3 * c, F32, 64)
    _C.check(lib.tok_bn_bwd_finalize(pg.ptr, rows, q['m'], c, cr, ga.ptr, mu.ptr, rs.ptr, dg.ptr if grads else None, db.ptr if grads else None,
                                     coef.ptr, acc, dzy, st), 'bwd_finalize')
    torch.cuda.synchronize()
    for g, what in ((pg, 'partial'), (ga, 'gamma'), (mu, 'mean'), (rs, 'rstd')):
        g.check(what)
    if not grads:
        assert (dg.untouched() and db.untouched()) or acc
        dg.check('dgamma'), db.check('dbeta')
        return _written(coef, 'coef').view(3, c), None, None
    return _written(coef, 'coef').view(3, c), _written(dg, 'dgamma'), _written(db, 'dbeta')


@pytest.mark.parametrize('c', sorted(R.FINALIZE_ROWS))
def test_finalize_kernels_vs_fp64(c):
    for rows in R.FINALIZE_ROWS[c]:
        for integer in (True, False):
            tag = f'bn_contract/finalize_c{c}_r{rows}_{"int" if integer else "real"}'
            p = R.finalize_rows(rows, c, integer)
            ref = R.FinalizeRef(p)
            assert bool((ref.var[2:] > 0).all())
            res = _finalize(p, c)
            assert all(torch.equal(a, b) for a, b in zip(res, _finalize(p, c)))
            ref.check(tag, *res)
            if integer:          # count = 256: the mean is S1 / count exactly
                assert torch.equal(res[0].double(), ref.S[0] / p['count'])
            else:
                assert abs(float(res[1][1]) - R.EPS ** -0.5) <= float(ref.b_rstd[1]) and float(ref.b_rstd[1]) <= 1e-6 * R.EPS ** -0.5
            q = R.bwd_rows(rows, c, integer)
            for dzy, acc in ((0, 0), (0, 1), (1, 0), (1, 1)):
                bref = R.BwdFinalizeRef(q, dzy, acc)
                coef, dg, db = _bwd_finalize(q, c, dzy, acc)
                bref.check(f'{tag}_dzy{dzy}_acc{acc}', coef, dg, db, exact_sums=integer and not dzy)
                if integer and dzy:          # dbeta is the integer sum in either form
                    assert torch.equal(db.double(), bref.dbeta)
            coef2, _, _ = _bwd_finalize(q, c, 0, 0, grads=False)
            assert torch.equal(coef2, _bwd_finalize(q, c, 0, 0)[0])
    # count = 1 (unbias = 1), no running statistics, c_real < c
    rows = R.FINALIZE_ROWS[c][4]
    p = R.finalize_rows(rows, c, False)
    R.FinalizeRef(p, count=1).check(f'bn_contract/finalize_c{c}_count1', *_finalize(p, c, count=1))
    R.FinalizeRef(p).check(f'bn_contract/finalize_c{c}_norunning', *_finalize(p, c, running=False))
    cr = c - 3
    R.FinalizeRef(p, c_real=cr).check(f'bn_contract/finalize_c{c}_creal', *_finalize(p, c, c_real=cr))
    q = R.bwd_rows(rows, c, False)
    for dzy, acc in ((0, 1), (1, 0)):
        R.BwdFinalizeRef(q, dzy, acc, c_real=cr).check(f'bn_contract/finalize_c{c}_creal_dzy{dzy}', *_bwd_finalize(q, c, dzy, acc, c_real=cr))


@pytest.mark.parametrize('m,c', [(777, 48), (1027, 2048)])
def test_chain_on_the_device_intermediates_vs_batch_norm_autograd(m, c):
    """tok_bn_stats -> tok_bn_finalize -> tok_bn_act_fwd -> tok_bn_bwd_reduce -> tok_bn_bwd_finalize -> tok_bn_bwd_apply, each fed
    what the one before wrote, against fp64 batch_norm (+ shortcut, ReLU) and its gradient: the only place the pieces meet"""
    lib, st = _C.lib(), stream_ptr()
    rows = _rows(m, c)
    d = R.stream_inputs(m, c, False, seed=2)
    g = torch.Generator().manual_seed(m + c)
    gamma, beta = 1.0 + 0.3 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)
    ref = R.ChainRef(d['y'], d['shortcut'], d['dout'], gamma, beta)
    y, sc, do = (gin(d[k], GUARD) for k in ('y', 'shortcut', 'dout'))
    ga, be = gin(gamma, 64), gin(beta, 64)
    stats, part = gout(2 * rows * c, F32, GUARD), gout(2 * rows * c, F32, GUARD)
    mean, rstd, scale, shift = (gout(c, F32, 64) for _ in range(4))
    out, dy, ds, mask = gout(m * c, BF, GUARD), gout(m * c, BF, GUARD), gout(m * c, BF, GUARD), gout(m * c // 8, U8, GUARD)
    coef, dg, db = gout(3 * c, F32, 64), gout(c, F32, 64), gout(c, F32, 64)
    _C.check(lib.tok_bn_stats(y.ptr, m, c, stats.ptr, st), 'stats')
    _C.check(lib.tok_bn_finalize(stats.ptr, rows, m, c, c, ga.ptr, be.ptr, None, None, None, R.MOMENTUM, R.EPS, mean.ptr, rstd.ptr,
                                 scale.ptr, shift.ptr, st), 'finalize')
    _C.check(lib.tok_bn_act_fwd(y.ptr, scale.ptr, shift.ptr, sc.ptr, 1, out.ptr, mask.ptr, m, c, st), 'act_fwd')
    _C.check(lib.tok_bn_bwd_reduce(do.ptr, y.ptr, mask.ptr, scale.ptr, shift.ptr, mean.ptr, rstd.ptr, 1, m, c, part.ptr, st), 'reduce')
    _C.check(lib.tok_bn_bwd_finalize(part.ptr, rows, m, c, c, ga.ptr, mean.ptr, rstd.ptr, dg.ptr, db.ptr, coef.ptr, 0, 0, st), 'bwd_finalize')
    _C.check(lib.tok_bn_bwd_apply(do.ptr, y.ptr, mask.ptr, scale.ptr, shift.ptr, coef.ptr, 1, dy.ptr, ds.ptr, 0, m, c, st), 'apply')
    torch.cuda.synchronize()
    for t in (y, sc, do, ga, be):
        t.check('input')
    for t, what in ((stats, 'stats'), (part, 'partial'), (mean, 'mean'), (rstd, 'rstd'), (scale, 'scale'), (shift, 'shift'), (coef, 'coef'),
                    (dg, 'dgamma'), (db, 'dbeta'), (ds, 'dshortcut')):
        _written(t, what)
    mask.check('mask')
    ref.check(f'bn_contract/chain_{m}x{c}', _written(out, 'out').view(m, c), _written(dy, 'dy').view(m, c))
    mu, rs, b_rstd, e_mu = ref.stats
    R.assert_bounded(mean.value(), mu, e_mu, 0.0, 1.0, 'chain mean')
    R.assert_bounded(rstd.value(), rs, b_rstd, 0.0, 1.0, 'chain rstd')


# ---- fused stem ------------------------------------------------------------------------------------------------------------
def _stem(d, tap8, with_ypool=True):
    """forward, then the three backward kernels on the tap indices `tap8` and the pooled / ypool tensors of the reference"""
    lib, st = _C.lib(), stream_ptr()
    n, h, w, c, p, q = d['dims']
    m, mp = n * h * w, n * p * q
    y, dp = gin(d['y'], GUARD), gin(d['dpool'], GUARD)
    v = {k: gin(d[k], 64) for k in ('scale', 'shift', 'mean', 'rstd', 'coef')}
    pooled, arg, ypool = gout(mp * c, BF, GUARD), gout(mp * c, U8, GUARD), gout(mp * c, BF, GUARD)
    _C.check(lib.tok_bn_relu_maxpool_fwd(y.ptr, v['scale'].ptr, v['shift'].ptr, n, h, w, c, pooled.ptr, arg.ptr,
                                         ypool.ptr if with_ypool else None, st), 'stem fwd')
    torch.cuda.synchronize()
    arg.check('argmax')
    r = dict(pooled=_written(pooled, 'pooled'), argmax=arg.value())
    if with_ypool:
        r['ypool'] = _written(ypool, 'ypool')
    else:
        ypool.check('ypool')
        assert ypool.untouched(), 'ypool == NULL: nothing is written for it'
        return r
    rows, rows_p = _rows(m, c), _rows(mp, c)
    tg = gin(tap8, GUARD)
    part, dy, part_p = gout(2 * rows * c, F32, GUARD), gout(m * c, BF, GUARD), gout(2 * rows_p * c, F32, GUARD)
    _C.check(lib.tok_bn_pool_bwd_reduce(dp.ptr, tg.ptr, y.ptr, v['scale'].ptr, v['shift'].ptr, v['mean'].ptr, v['rstd'].ptr, n, h, w, c,
                                        part.ptr, st), 'pool reduce')
    _C.check(lib.tok_bn_pool_bwd_apply(dp.ptr, tg.ptr, y.ptr, v['scale'].ptr, v['shift'].ptr, v['coef'].ptr, n, h, w, c, dy.ptr, st),
             'pool apply')
    pin, yin = gin(d['pooled_in'], GUARD), gin(d['ypool_in'], GUARD)
    _C.check(lib.tok_bn_pool_bwd_reduce_pooled(dp.ptr, pin.ptr, yin.ptr, v['mean'].ptr, v['rstd'].ptr, mp, c, part_p.ptr, st), 'pooled reduce')
    torch.cuda.synchronize()
    for g in [y, dp, tg, pin, yin] + list(v.values()):
        g.check('stem input')
    r.update(part=_written(part, 'pool partial').view(2, rows, c), dy=_written(dy, 'pool dy').view(m, c),
             part_p=_written(part_p, 'pooled partial').view(2, rows_p, c))
    return r


@pytest.mark.parametrize('n,h,w,c', R.STEM_SHAPES)
def test_fused_stem_vs_fp64(n, h, w, c):
    for integer in (True, False):
        tag = f'bn_contract/stem_{n}x{h}x{w}x{c}_{"int" if integer else "real"}'
        d = R.stem_inputs(n, h, w, c, integer)
        p, q = d['dims'][4:]
        m, mp = n * h * w, n * p * q
        ref = R.StemRef(d)
        b = ref.bwd(d, ref.tap)
        d['pooled_in'], d['ypool_in'] = R.bf(ref.pooled).reshape(mp, c), ref.ypool.reshape(mp, c).contiguous()
        tap8 = ref.tap.to(torch.uint8).reshape(mp, c).contiguous()
        r = _stem(d, tap8)
        _same(r, _stem(d, tap8), 'stem')
        R.check_stem_fwd(tag, d, ref, r['pooled'], r['argmax'], r['ypool'], integer)
        if integer:
            assert 2 * float(b['m_sums'].max()) < 2 ** 24
        R.check_stem_bwd(tag, b, m, c, r['part'].double().sum(1), r['dy'], integer)
        ps, pm = ref.pooled_sums(d, d['pooled_in'], d['ypool_in'])
        R.check_sums(tag, 'pooled_reduce', r['part_p'].double().sum(1), ps, pm, torch.zeros(2, c), R.n_sum(mp, c), integer)
        nop = _stem(d, tap8, with_ypool=False)
        assert torch.equal(nop['pooled'], r['pooled']) and torch.equal(nop['argmax'], r['argmax'])


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_function_and_write_nothing():
    lib, st = _C.lib(), stream_ptr()
    buf = torch.zeros(4096, device='cuda')
    p = buf.data_ptr()
    outs = [gout(1024, BF, 64) for _ in range(3)] + [gout(1024, F32, 64) for _ in range(4)] + [gout(1024, U8, 64)]
    o = [g.ptr for g in outs[:3]]
    f = [g.ptr for g in outs[3:7]]
    u = outs[7].ptr

    def refused(name, rc):
        assert rc == ERR_INVALID, f'{name} returned {rc}'
        assert name in last_error(), (name, last_error())

    for m, c in ((4, 12), (0, 8), (-1, 8), (4, 0)):          # c % 8 != 0, m <= 0
        refused('tok_bn_stats', lib.tok_bn_stats(p, m, c, f[0], st))
        refused('tok_bn_act_fwd', lib.tok_bn_act_fwd(p, p, p, None, 1, o[0], u, m, c, st))
        refused('tok_bn_act_fwd_colsum', lib.tok_bn_act_fwd_colsum(p, p, p, None, 1, o[0], u, m, c, f[0], st))
        refused('tok_bn_bwd_reduce', lib.tok_bn_bwd_reduce(p, p, None, p, p, p, p, 0, m, c, f[0], st))
        refused('tok_bn_bwd_apply', lib.tok_bn_bwd_apply(p, p, None, p, p, p, 0, o[0], o[1], 0, m, c, st))
        refused('tok_bn_relu_maxpool_fwd', lib.tok_bn_relu_maxpool_fwd(p, p, p, 1, 2, max(m, 0), c, o[0], u, o[1], st))
        refused('tok_bn_pool_bwd_reduce', lib.tok_bn_pool_bwd_reduce(p, p, p, p, p, p, p, 1, 2, max(m, 0), c, f[0], st))
        refused('tok_bn_pool_bwd_apply', lib.tok_bn_pool_bwd_apply(p, p, p, p, p, p, 1, 2, max(m, 0), c, o[0], st))
        refused('tok_bn_pool_bwd_reduce_pooled', lib.tok_bn_pool_bwd_reduce_pooled(p, p, p, p, p, m, c, f[0], st))
    refused('tok_bn_act_fwd_colsum', lib.tok_bn_act_fwd_colsum(p, p, p, None, 1, o[0], u, 1, 2176, f[0], st))
    # a null pointer
    refused('tok_bn_stats', lib.tok_bn_stats(None, 4, 8, f[0], st))
    refused('tok_bn_act_fwd', lib.tok_bn_act_fwd(p, None, p, None, 1, o[0], u, 4, 8, st))
    refused('tok_bn_act_fwd_colsum', lib.tok_bn_act_fwd_colsum(p, p, p, None, 1, o[0], u, 4, 8, None, st))
    refused('tok_bn_bwd_reduce', lib.tok_bn_bwd_reduce(p, p, None, p, p, None, p, 0, 4, 8, f[0], st))
    refused('tok_bn_bwd_apply', lib.tok_bn_bwd_apply(p, p, None, p, p, None, 0, o[0], o[1], 0, 4, 8, st))
    refused('tok_bn_finalize', lib.tok_bn_finalize(p, 1, 4, 8, 8, None, p, None, None, None, 0.1, 1e-5, *f, st))
    refused('tok_bn_bwd_finalize', lib.tok_bn_bwd_finalize(p, 1, 4, 8, 8, p, None, p, f[0], f[1], f[2], 0, 0, st))
    refused('tok_bn_relu_maxpool_fwd', lib.tok_bn_relu_maxpool_fwd(p, p, p, 1, 2, 2, 8, o[0], None, o[1], st))
    refused('tok_bn_pool_bwd_reduce', lib.tok_bn_pool_bwd_reduce(p, None, p, p, p, p, p, 1, 2, 2, 8, f[0], st))
    refused('tok_bn_pool_bwd_apply', lib.tok_bn_pool_bwd_apply(p, p, p, p, p, None, 1, 2, 2, 8, o[0], st))
    refused('tok_bn_pool_bwd_reduce_pooled', lib.tok_bn_pool_bwd_reduce_pooled(p, p, None, p, p, 4, 8, f[0], st))
    # relu with a shortcut gradient and no mask
    refused('tok_bn_bwd_apply', lib.tok_bn_bwd_apply(p, p, None, p, p, p, 1, o[0], o[1], 0, 4, 8, st))
    # c_real > c, and sizes of the finalize kernels (rows <= 0, count or m <= 0)
    for rows, cnt, c, cr in ((1, 4, 8, 9), (1, 4, 8, 0), (0, 4, 8, 8), (-1, 4, 8, 8), (1, 0, 8, 8), (1, -2, 8, 8), (1, 4, 0, 0)):
        refused('tok_bn_finalize', lib.tok_bn_finalize(p, rows, cnt, c, cr, p, p, None, None, None, 0.1, 1e-5, *f, st))
        refused('tok_bn_bwd_finalize', lib.tok_bn_bwd_finalize(p, rows, cnt, c, cr, p, p, p, f[0], f[1], f[2], 0, 0, st))
    refused('tok_bn_finalize', lib.tok_bn_finalize(p, 1, 4, 8, 8, p, p, f[3], None, None, 0.1, 1e-5, *f, st))      # one running array only
    torch.cuda.synchronize()
    for g in outs:
        g.check('refused call')
        assert g.untouched(), 'a refused call wrote to an output'
