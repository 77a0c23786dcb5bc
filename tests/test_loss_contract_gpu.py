"""The loss entries of csrc/loss_*.hip and the metric-count entries of csrc/metric.hip element by element against fp64 of the same bf16 inputs; references, bounds
and input makers are in tests/loss_ref.py (tests/test_loss_ref.py: an fp32 run stays inside half of every bound).

Every case states which kernel or reduction class it is meant to run, and asserts it against a restatement of the launcher's
rule, so that a threshold change moves a test instead of silently moving coverage:
  softmax CE     wave kernel / thread-per-row kernel (ld <= 64, ld % 8 == 0, rows >= 16384, 16-byte aligned; the backward also
                 needs dlogits aligned), reduction into 1 part / several / the 512-part cap with a ragged chunk
  upsample CE    tiled backward (destination / source ratio <= 4) / gather backward, per geometry
  Dice           one trip / a second grid-stride trip with an odd remainder / many trips
  BCE, regression   1 part / several / capped; the backward's 4096-block cap
  counts         one trip / grid-stride trips of the 2048-block grid
Inputs sit behind NaN pads and guards, outputs carry sentinels (pad columns that the contract zeroes are asserted zero), every
owned output element is written.  The worst |err| / bound of every tensor of every kernel family goes to the parity record
(profiles/loss_contract_parity_distances.json; profiles/loss_contract_mutation_check.txt: nine hand-made kernel defects, each seen).

Upsample CE: 149 357 of the 2 739 600 interpolated logits of test_upsample_ce_geometries (5.5 %) take the rounding-tie slack of
loss_ref.UpRef: at power-of-two ratios the weights are multiples of 1/8, and a mean of neighbouring bf16 values IS a rounding tie
(16x16 -> 16x16: 0.6 %); the dyadic case, where the fp32 interpolant is proven exact, takes none.

On an MI355X the module runs in 9 s; the slowest case is test_softmax_ce_reduction_split[2101249-capped], 1.4 s (2.1 M rows, two
ignore indices x three smoothing values), then the 4.2 M-element regression cases, 0.5 s each."""
import math

import pytest
import torch

from helpers import A_BF, BF, ERR_INVALID, F32, SENTINEL, U32, GuardedSpan, Mat, cdiv
import loss_ref as L
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
P = lambda t: None if t is None else t.data_ptr()       # noqa: E731


@pytest.fixture(autouse=True, scope='module')
def _parity_record():
    """one line per kernel family and tensor: the worst |err| / bound over every case and variant of the family"""
    yield
    L.flush_record()


LOSS_FLOATS = 2050          # TOK_CE_LOSS_FLOATS
CE_PARTS = 512


def _loss_buf():
    return GuardedSpan(LOSS_FLOATS, F32, 64)


def _gs(v):
    return None if v is None else torch.tensor([v], dtype=F32, device='cuda')


# ---- softmax cross entropy ----------------------------------------------------------------------------------------------------------
def ce_small(ptr, rows, ld):
    return ld <= 64 and ld % 8 == 0 and rows >= 16384 and ptr % 16 == 0


def ce_parts(rows, chunk_rows=4096):
    return 1 if rows < chunk_rows else min(cdiv(rows, chunk_rows), CE_PARTS)


def _ce(tag, rows, classes, ld, kernels, parts, off_z=0, off_d=0, all_ignored=False, ignores=(-100, 255), on_device=False):
    """kernels: (forward, backward) in 'wave' / 'small'; parts: '1' / 'several' / 'capped'"""
    lib, st = _C.lib(), stream_ptr()
    for ign in ignores:
        z, t = L.make_ce(rows, classes, ign, seed=rows + classes)
        if all_ignored:
            t[:] = ign
        zc, tc = z.cuda(), t.cuda()
        zg = Mat(rows, classes, ld, init=zc, nan=True, off=off_z)
        assert ('small' if ce_small(zg.ptr, rows, ld) else 'wave') == kernels[0]
        np_ = ce_parts(rows)
        assert ('1' if np_ == 1 else 'several' if cdiv(rows, 4096) < CE_PARTS else 'capped') == parts
        for s in (0.0, 0.1, 1.0):
            ref = L.CERef(zc if on_device else z, tc if on_device else t, ign, s)
            lg, rg, lo = Mat(1, rows, dtype=F32), Mat(1, rows, dtype=F32), _loss_buf()
            _C.check(lib.tok_softmax_ce_smooth_fwd(zg.ptr, P(tc), rows, classes, ld, ign, s, lg.ptr, rg.ptr, lo.ptr, st), 'fwd')
            torch.cuda.synchronize()
            zg.done('logits', finite=False)
            lg.done('lse')
            rg.done('row_loss', finite=not bool(ref.inf_rows.any()))
            lo.check('loss')
            L.check_ce_fwd(tag, ref, lg.view[0], rg.view[0])
            L.check_ce_mean(tag, ref, lo.view[:2], rg.view[0])
            l32 = ref.lse32.cuda()
            outs = []
            for gs in ((0.7, None) if s == 0.0 else (0.7,)):
                dg = Mat(rows, classes, ld, off=off_d)
                assert ('small' if ce_small(zg.ptr, rows, ld) and dg.ptr % 16 == 0 else 'wave') == kernels[1]
                _C.check(lib.tok_softmax_ce_smooth_bwd(zg.ptr, P(tc), P(l32), lo.ptr, P(_gs(gs)), rows, classes, ld, ign, s, dg.ptr, st), 'bwd')
                torch.cuda.synchronize()
                dg.done('dlogits', zero_pads=True)
                L.check_ce_bwd(tag, ref, 1.0 if gs is None else gs, dg.view)
                outs.append(dg)
            if s == 0.0:
                # s = 0 is tok_softmax_ce_fwd / _bwd bit for bit (include/tok.h)
                lg2, rg2, lo2, dg2 = Mat(1, rows, dtype=F32), Mat(1, rows, dtype=F32), _loss_buf(), Mat(rows, classes, ld, off=off_d)
                _C.check(lib.tok_softmax_ce_fwd(zg.ptr, P(tc), rows, classes, ld, ign, lg2.ptr, rg2.ptr, lo2.ptr, st), 'plain fwd')
                _C.check(lib.tok_softmax_ce_bwd(zg.ptr, P(tc), P(l32), lo2.ptr, P(_gs(0.7)), rows, classes, ld, ign, dg2.ptr, st), 'plain bwd')
                torch.cuda.synchronize()
                i32 = lambda q: q.view(torch.int32)          # noqa: E731
                assert torch.equal(i32(lg2.view), i32(lg.view)) and torch.equal(i32(rg2.view), i32(rg.view))
                assert torch.equal(i32(lo2.view[:2]), i32(lo.view[:2])) and torch.equal(dg2.full.view(torch.int16), outs[0].full.view(torch.int16))
            if all_ignored:
                assert float(lo.view[1]) == 0 and math.isnan(float(lo.view[0]))
                assert bool((outs[0].view == 0).all())


WAVE = [(7, 10, 10), (5, 1, 8), (37, 63, 64), (37, 64, 64), (37, 65, 72), (33, 1000, 1000), (9, 1001, 1008)]


@pytest.mark.parametrize('rows,classes,ld', WAVE)
def test_softmax_ce_wave_kernel(rows, classes, ld):
    _ce('loss_contract/ce_wave_kernel', rows, classes, ld, ('wave', 'wave'), '1')


@pytest.mark.parametrize('rows,classes,ld,kernel', [(16383, 3, 8, 'wave'), (16384, 3, 8, 'small'), (16383, 19, 24, 'wave'),
                                                     (16384, 19, 24, 'small'), (16641, 33, 40, 'small'), (16641, 63, 64, 'small'),
                                                     (16641, 64, 64, 'small')])
def test_softmax_ce_thread_per_row_kernel(rows, classes, ld, kernel):
    _ce(f'loss_contract/ce_thread_per_row_{kernel}', rows, classes, ld, (kernel, kernel), 'several', on_device=True)


def test_softmax_ce_misaligned_pointers_fall_back_to_the_wave_kernel():
    _ce('loss_contract/ce_misaligned', 16641, 19, 24, ('wave', 'wave'), 'several', off_z=4, ignores=(255,), on_device=True)
    _ce('loss_contract/ce_misaligned', 16641, 19, 24, ('small', 'wave'), 'several', off_d=4, ignores=(255,), on_device=True)


@pytest.mark.parametrize('rows,parts', [(4095, '1'), (4096, '1'), (4097, 'several'), (512 * 4096 + 4097, 'capped')])
def test_softmax_ce_reduction_split(rows, parts):
    """4096 rows still make one part (cdiv = 1); the last case crosses the 512-part cap: chunks of 4105 rows, the last ragged"""
    _ce('loss_contract/ce_reduction_split', rows, 3, 8, ('small' if rows >= 16384 else 'wave',) * 2, parts, on_device=True)


def test_softmax_ce_all_rows_ignored():
    _ce('loss_contract/ce_all_ignored', 37, 19, 24, ('wave', 'wave'), '1', all_ignored=True)


# ---- cross entropy on upsampled logits ------------------------------------------------------------------------------------------------
WIDTHS = [(3, 8), (8, 8), (13, 16), (19, 24), (25, 32), (32, 32)]
GEOM = [(2, 8, 8, 32, 32, 'tiled'), (2, 8, 8, 33, 33, 'gather'), (2, 4, 6, 32, 48, 'gather'), (2, 8, 4, 16, 32, 'gather'),
        (2, 9, 13, 36, 52, 'tiled'), (2, 3, 5, 12, 20, 'tiled'), (2, 1, 7, 4, 28, 'tiled'), (2, 16, 16, 16, 16, 'tiled'),
        (2, 16, 24, 8, 12, 'tiled'), (2, 16, 16, 5, 5, 'tiled'), (3, 17, 17, 68, 68, 'tiled')]


def _up(tag, n, hs, ws, hd, wd, classes, ld, kernel, dyadic=False, gs=1.3):
    lib, st = _C.lib(), stream_ptr()
    assert ('tiled' if L.up_tiled_ok(hs, ws, hd, wd) else 'gather') == kernel
    assert lib.tok_upsample_ce_serves(classes, ld) == 1
    low, t = L.make_up(n, hs, ws, classes, hd, wd, seed=hs + wd + classes, dyadic=dyadic)
    ref = L.UpRef(low, t, hd, wd, 255, gs=1.0 if gs is None else gs, exact=dyadic)
    rows, tc = n * hd * wd, t.cuda()
    zg = Mat(n * hs * ws, classes, ld, init=low.cuda(), nan=True)       # (NaN pad channels: loaded as whole vectors, never used)
    lg, rg, lo = Mat(1, rows, dtype=F32), Mat(1, rows, dtype=F32), _loss_buf()
    _C.check(lib.tok_upsample_ce_fwd(zg.ptr, n, hs, ws, classes, ld, hd, wd, P(tc), 255, lg.ptr, rg.ptr, lo.ptr, st), 'fwd')
    torch.cuda.synchronize()
    zg.done('low')
    lg.done('lse')
    rg.done('row_loss')
    lo.check('loss')
    L.check_ce_fwd(tag, ref.ce, lg.view[0], rg.view[0])
    L.check_ce_mean(tag, ref.ce, lo.view[:2], rg.view[0])
    l32 = ref.ce.lse32.cuda()
    prev = L.bf(torch.randn(n, hs, ws, ld, generator=torch.Generator().manual_seed(1)))
    for acc in (0, 1):
        dg = Mat(n * hs * ws, ld, ld, init=(prev if acc else torch.full((n, hs, ws, ld), 9.0)).cuda())
        _C.check(lib.tok_upsample_ce_bwd(zg.ptr, n, hs, ws, classes, ld, hd, wd, P(tc), 255, P(l32), lo.ptr, P(_gs(gs)), dg.ptr, acc, st), 'bwd')
        torch.cuda.synchronize()
        dg.span.check('dlow')
        d = dg.value().view(n, hs, ws, ld)
        assert bool(torch.isfinite(d.float()).all())
        ref.check_bwd(tag, d[..., :classes], prev=prev[..., :classes] if acc else None)
        if acc:
            assert torch.equal(d[..., classes:], prev[..., classes:]), 'pad channels: nothing to add'
        else:
            assert bool((d[..., classes:] == 0).all()), 'pad channels are zero when fresh'
            assert bool((d[:, ref.unmapped][..., :classes] == 0).all()), 'a source pixel no destination maps to gets 0'
    return ref


@pytest.mark.parametrize('n,hs,ws,hd,wd,kernel', GEOM)
def test_upsample_ce_geometries(n, hs, ws, hd, wd, kernel):
    slack = 0
    for i, (classes, ld) in enumerate(WIDTHS):
        ref = _up(f'loss_contract/upce_{kernel}', n, hs, ws, hd, wd, classes, ld, kernel, gs=None if i == 1 else 1.3)
        slack += ref.n_slack
        if (hd, wd) == (5, 5):
            assert bool(ref.unmapped.any())          # (halving maps every source pixel, with weight 1/2; 16 -> 5 skips every third)
    print(f'upsample CE {hs}x{ws} -> {hd}x{wd}: {slack} interpolated logits took the rounding-tie slack')


def test_upsample_ce_exact_case_takes_no_slack():
    """dyadic inputs, power-of-two scales: the fp32 interpolant is exact, so no element may use the tie slack (tiled and gather)"""
    for hs, ws, hd, wd, kernel in ((8, 8, 32, 32, 'tiled'), (4, 8, 32, 64, 'gather')):
        ref = _up(f'loss_contract/upce_dyadic_{kernel}', 2, hs, ws, hd, wd, 19, 24, kernel, dyadic=True)
        assert ref.n_slack == 0


@pytest.mark.parametrize('classes,ld', [(33, 40), (9, 12)])
def test_upsample_ce_refusals(classes, ld):
    lib, st = _C.lib(), stream_ptr()
    n, hs, ws, hd, wd = 1, 4, 4, 8, 8
    assert lib.tok_upsample_ce_serves(classes, ld) == 0
    zg = Mat(n * hs * ws, ld, ld, init=torch.zeros(n * hs * ws, ld).cuda(), nan=True)
    t = torch.zeros(n, hd, wd, dtype=torch.int64, device='cuda')
    lg, rg, lo, dg = Mat(1, n * hd * wd, dtype=F32), Mat(1, n * hd * wd, dtype=F32), _loss_buf(), Mat(n * hs * ws, ld, ld)
    assert lib.tok_upsample_ce_fwd(zg.ptr, n, hs, ws, classes, ld, hd, wd, P(t), 255, lg.ptr, rg.ptr, lo.ptr, st) == ERR_INVALID
    l32, l2 = torch.zeros(n * hd * wd, device='cuda'), torch.ones(LOSS_FLOATS, device='cuda')
    assert lib.tok_upsample_ce_bwd(zg.ptr, n, hs, ws, classes, ld, hd, wd, P(t), 255, P(l32), P(l2), None, dg.ptr, 0, st) == ERR_INVALID
    torch.cuda.synchronize()
    for m, what in ((lg, 'lse'), (rg, 'row_loss'), (dg, 'dlow')):
        m.intact(what)
    assert lo.untouched()


# ---- Dice ---------------------------------------------------------------------------------------------------------------------------
def _dice(tag, mode, rows, classes, ld, trips):
    lib, st = _C.lib(), stream_ptr()
    g = lib.tok_dice_rows(rows)
    assert g == L.dice_rows(rows)
    assert {1: 'one', 2: 'two'}.get(cdiv(rows, 4 * g), 'many') == trips
    empty = 1 if classes > 2 else None
    z, t = L.make_dice(rows, classes, mode, seed=rows + mode, empty_class=empty)
    ref = L.DiceRef(z.cuda(), t.cuda(), mode, g)
    zg = Mat(rows, classes, ld, init=z.cuda(), nan=True)
    tg = t.cuda() if mode == 0 else GuardedSpan(t.numel(), F32, 256, init=t.cuda(), nan_guard=True)
    tp = P(tg) if mode == 0 else tg.ptr
    sels = [None] if classes <= 2 else [None, [0, classes - 1], [0, 1, classes - 1]]
    for log_loss in (0, 1):
        for smooth in (0.0, 1.0):
            for sel in sels:
                sc = None if sel is None else torch.tensor(sel, device='cuda')
                pg, lo, cg = Mat(3 * g, classes, dtype=F32), GuardedSpan(1, F32, 64), Mat(2, classes, dtype=F32)
                _C.check(lib.tok_dice_fwd(zg.ptr, tp, rows, classes, ld, mode, smooth, 1e-7, log_loss, P(sc), 0 if sel is None else len(sel),
                                          pg.ptr, lo.ptr, cg.ptr, st), 'fwd')
                torch.cuda.synchronize()
                zg.done('logits', finite=False)
                pg.done('partial')
                cg.done('coef')
                lo.check('loss')
                assert not lo.untouched() and math.isfinite(float(lo.view[0]))
                part = pg.view.double().view(g, 3, classes).sum(0)
                assert torch.equal(part[2], ref.Y), 'Y is an exact integer sum'
                L.bounded(part[0], ref.I, ref.m_I, 0.0, U32, 'I', tag)
                L.bounded(part[1], ref.P, ref.m_P, 0.0, U32, 'P', tag)
                # finalize alone, on the kernel's own sums
                l64, m_l, c64 = ref.finalize(part[0].cpu(), part[1].cpu(), part[2].cpu(), smooth, 1e-7, log_loss, sel)
                L.bounded(lo.view[:1], l64.reshape(1), m_l.reshape(1), 0.0, U32, 'loss', tag)
                L.bounded(cg.view, c64, c64.abs(), 0.0, ref.K_FIN * U32, 'coef', tag)
                if empty is not None:
                    assert float(cg.view[0, empty]) == 0 and float(cg.view[1, empty]) == 0, 'a class without true pixels contributes nothing'
                for gs in (0.9, None):
                    dg = Mat(rows, classes, ld)
                    _C.check(lib.tok_dice_bwd(zg.ptr, tp, cg.ptr, P(_gs(gs)), rows, classes, ld, mode, dg.ptr, st), 'bwd')
                    torch.cuda.synchronize()
                    dg.done('dlogits', zero_pads=True)
                    gv = 1.0 if gs is None else gs
                    # against the fp64 formula fed the kernel's own coef, then end to end
                    w, mag = ref.grad(cg.view.double(), gv)
                    L.bounded(dg.view, w, mag, A_BF, U32, 'dlogits of its own coef', tag)
                    l64, m_l, c64 = ref.finalize(ref.I.cpu(), ref.P.cpu(), ref.Y.cpu(), smooth, 1e-7, log_loss, sel)
                    w, mag = ref.grad(c64.cuda(), gv, ref.coef_rel().cuda())
                    L.bounded(dg.view, w, mag, A_BF, U32, 'dlogits end to end', tag)
                    if sel is not None or log_loss or smooth:
                        break                                            # gscale = NULL once per shape and mode


@pytest.mark.parametrize('mode', [0, 2])
@pytest.mark.parametrize('rows,classes,ld,trips', [(777, 5, 8, 'one'), (5000, 19, 24, 'one'), (8192, 63, 64, 'one'), (8193, 64, 64, 'two'),
                                                   (100003, 19, 24, 'many')])
def test_dice(mode, rows, classes, ld, trips):
    _dice(f'loss_contract/dice_m{mode}', mode, rows, classes, ld, trips)


def test_dice_binary():
    _dice('loss_contract/dice_m1', 1, 4099, 1, 8, 'one')


def test_dice_refusals():
    lib, st = _C.lib(), stream_ptr()
    rows = 16
    zg = Mat(rows, 72, 72, init=torch.zeros(rows, 72).cuda(), nan=True)
    t, sel = torch.zeros(rows, dtype=torch.int64, device='cuda'), torch.zeros(4, dtype=torch.int64, device='cuda')
    pg, lo, cg, dg = Mat(3 * 4, 72, dtype=F32), GuardedSpan(1, F32, 64), Mat(2, 72, dtype=F32), Mat(rows, 72, 72)
    assert lib.tok_dice_fwd(zg.ptr, P(t), rows, 5, 8, 0, 0.0, 1e-7, 0, P(sel), 0, pg.ptr, lo.ptr, cg.ptr, st) == ERR_INVALID
    assert lib.tok_dice_fwd(zg.ptr, P(t), rows, 65, 72, 0, 0.0, 1e-7, 0, None, 0, pg.ptr, lo.ptr, cg.ptr, st) == ERR_INVALID
    assert lib.tok_dice_bwd(zg.ptr, P(t), cg.ptr, None, rows, 65, 72, 0, dg.ptr, st) == ERR_INVALID
    torch.cuda.synchronize()
    for m, what in ((pg, 'partial'), (cg, 'coef'), (dg, 'dlogits')):
        m.intact(what)
    assert lo.untouched()


# ---- BCE with logits ------------------------------------------------------------------------------------------------------------------
def el_parts(n):
    return 1 if n < 8192 else min(cdiv(n, 8192), CE_PARTS)


def _parts_class(n):
    return '1' if el_parts(n) == 1 else 'several' if cdiv(n, 8192) < CE_PARTS else 'capped'


@pytest.mark.parametrize('rows,classes,ld,mean,parts,bwd_capped', [(37, 21, 24, 1, '1', False), (5, 1, 8, 0, '1', False),
                                                                   (1171, 7, 8, 1, 'several', False), (70001, 16, 16, 0, 'several', True),
                                                                   (600000, 7, 8, 1, 'capped', True)])
def test_bce_logits(rows, classes, ld, mean, parts, bwd_capped):
    lib, st = _C.lib(), stream_ptr()
    assert _parts_class(rows * classes) == parts and (cdiv(rows * ld, 256) > 4096) == bwd_capped
    tag = 'loss_contract/bce'
    z, t = L.make_bce(rows, classes, -1.0, seed=rows)
    for everything_ignored in (False, True):
        if everything_ignored:
            t[:] = -1.0
        zc, tc = z.cuda(), t.cuda()
        loss64, b_loss, n, d64, mag = L.bce_ref(zc, tc, -1.0, mean, 1.7)
        zg = Mat(rows, classes, ld, init=zc, nan=True)
        tg = GuardedSpan(t.numel(), F32, 256, init=tc, nan_guard=True)
        lo, dg = _loss_buf(), Mat(rows, classes, ld)
        _C.check(lib.tok_bce_logits_fwd(zg.ptr, tg.ptr, rows, classes, ld, -1.0, mean, lo.ptr, st), 'fwd')
        _C.check(lib.tok_bce_logits_bwd(zg.ptr, tg.ptr, lo.ptr, P(_gs(1.7)), rows, classes, ld, -1.0, mean, dg.ptr, st), 'bwd')
        torch.cuda.synchronize()
        zg.done('logits', finite=False)
        tg.check('target')
        lo.check('loss')
        dg.done('dlogits', zero_pads=True)
        assert float(lo.view[1]) == n
        L.bounded(lo.view[:1], loss64.reshape(1), b_loss.reshape(1), 0.0, 1.0, 'loss', tag)
        L.bounded(dg.view, d64, mag, A_BF, U32, 'dlogits', tag)
        if everything_ignored:
            assert n == 0 and float(lo.view[0]) == 0 and bool((dg.view == 0).all()), 'nothing selected: loss 0, gradient 0'
        if rows > 100000:
            break


# ---- regression losses ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [0, 1, 2, 3])
@pytest.mark.parametrize('n,parts', [(1, '1'), (8191, '1'), (8192, '1'), (8193, 'several'), (1048577, 'several'), (512 * 8192 + 8193, 'capped')])
def test_regression_losses(n, parts, kind):
    lib, st = _C.lib(), stream_ptr()
    assert _parts_class(n) == parts
    for knee in (0.5, 1.5):
        x, t = L.make_reg(n, knee, seed=n + kind)
        xc, tc = x.cuda(), t.cuda()
        xg = GuardedSpan(n, BF, 256, init=xc, nan_guard=True)
        tg = GuardedSpan(n, F32, 256, init=tc, nan_guard=True)
        for mean in (0, 1):
            name = f'loss_contract/reg_k{kind}'
            loss64, b_loss, d64, mag = L.reg_ref(xc, tc, kind, knee, mean, 1.3)
            lo, dg = _loss_buf(), GuardedSpan(n, BF, 256)
            _C.check(lib.tok_regression_loss_fwd(xg.ptr, tg.ptr, n, kind, knee, mean, lo.ptr, st), 'fwd')
            _C.check(lib.tok_regression_loss_bwd(xg.ptr, tg.ptr, P(_gs(1.3)), n, kind, knee, mean, dg.ptr, st), 'bwd')
            torch.cuda.synchronize()
            for s_, what in ((xg, 'x'), (tg, 'target'), (lo, 'loss'), (dg, 'dx')):
                s_.check(what)
            assert int((dg.view.view(torch.int16) == SENTINEL[BF]).sum()) == 0 and bool(torch.isfinite(dg.view.float()).all())
            assert float(lo.view[1]) == n
            L.bounded(lo.view[:1], loss64.reshape(1), b_loss.reshape(1), 0.0, 1.0, 'loss', name)
            L.bounded(dg.view, d64, mag, A_BF, U32, 'dx', name)


def test_regression_refusals():
    lib, st = _C.lib(), stream_ptr()
    n = 64
    x, t = torch.zeros(n, dtype=BF, device='cuda'), torch.zeros(n, device='cuda')
    lo, dg, gs = _loss_buf(), GuardedSpan(n, BF, 256), _gs(1.0)
    for kind, knee in ((2, 0.0), (3, 0.0), (4, 1.0)):
        assert lib.tok_regression_loss_fwd(P(x), P(t), n, kind, knee, 1, lo.ptr, st) == ERR_INVALID
    assert lib.tok_regression_loss_bwd(P(x), P(t), P(gs), n, 4, 1.0, 1, dg.ptr, st) == ERR_INVALID
    torch.cuda.synchronize()
    assert lo.untouched() and dg.untouched()


# ---- metric counts --------------------------------------------------------------------------------------------------------------------
GUARD = 0x5A5B5C5D5E5F


# rows x classes; 70001 x 1000 would be a 140 MB operand: 20001 rows there, still three trips of the 2048-block grid
COUNTS = [(rows, classes) for rows in (7, 8193, 70001) for classes in (1, 3, 19, 64, 65, 1000) if rows * classes < 20e6] + [(20001, 1000)]


@pytest.mark.parametrize('rows,classes', COUNTS)
def test_metric_counts(rows, classes):
    """exact against numpy / bincount.  Rows 5 and 6 are all -inf: prediction 0, as torch.argmax; predicted labels hold classes, -1
    and 2^40 + 1 (in no column, the row still counts as actual)."""
    lib, st = _C.lib(), stream_ptr()
    trips = 'one' if rows == 7 else 'many'
    assert ('one' if cdiv(rows, 4) <= 2048 else 'many') == trips
    ld = cdiv(classes, 8) * 8
    z, lab, t = L.make_counts(rows, classes, 255, seed=rows + classes)
    zg = Mat(rows, classes, ld, init=z.cuda(), nan=True)
    labc, tc = lab.cuda(), t.cuda()
    for pred, args in ((z, (zg.ptr, None)), (lab, (None, P(labc)))):
        counts, conf = L.counts_ref(pred, t, classes, 255)
        if pred is z and rows > 6:
            assert int(conf[classes - 1, 0]) >= 1                       # the -inf row with target classes - 1
        cb = torch.full((3 * classes + 16,), GUARD, dtype=torch.int64, device='cuda')
        fb = torch.full((classes * classes + 16,), GUARD, dtype=torch.int64, device='cuda')
        cb[8:-8], fb[8:-8] = 5, 3                                       # accumulation onto non-zero counts, over two calls
        for _ in range(2):
            _C.check(lib.tok_cls_stats_update(*args, P(tc), rows, classes, ld, 255, cb.data_ptr() + 64, st), 'cls_stats')
            _C.check(lib.tok_confusion_update(*args, P(tc), rows, classes, ld, 255, fb.data_ptr() + 64, st), 'confusion')
        torch.cuda.synchronize()
        zg.done('logits', finite=False)
        for b in (cb, fb):
            assert bool((b[:8] == GUARD).all()) and bool((b[-8:] == GUARD).all()), 'guard overwritten'
        assert torch.equal(cb[8:-8].cpu().view(3, classes), 5 + 2 * counts), 'counts'
        assert torch.equal(fb[8:-8].cpu().view(classes, classes), 3 + 2 * conf), 'confusion'
