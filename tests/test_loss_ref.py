"""The references and bounds of tests/loss_ref.py: the fp64 references agree with torch's own cross_entropy (with label_smoothing),
F.interpolate + cross_entropy, binary_cross_entropy_with_logits, l1 / mse / smooth_l1 / huber and with the fake backend; a plain
fp32 run of the same formulas stays inside HALF of every bound at every shape class of tests/test_loss_contract_gpu.py (the large
ones reduced, every dispatch class kept), so an exact fp32 kernel passes that module; and three deliberately wrong fp32 variants
do NOT pass: s / ld in place of s / classes, the mean over all rows in place of the valid rows, and the interpolation weights of
y0 and y1 exchanged."""
import math

import pytest
import torch
import torch.nn.functional as F

from fake_backend import FakeTok
from helpers import A_BF, BF, U32, assert_bounded
import loss_ref as L

P = lambda t: None if t is None else t.data_ptr()       # noqa: E731
CE_SHAPES = [(7, 10, 10), (5, 1, 8), (37, 63, 64), (37, 64, 64), (37, 65, 72), (33, 1000, 1000), (9, 1001, 1008),
             (4097, 3, 8), (1031, 19, 24), (1031, 33, 40), (1031, 63, 64), (1031, 64, 64)]
UP_GEOM = [(8, 8, 32, 32), (8, 8, 33, 33), (4, 6, 32, 48), (8, 4, 16, 32), (9, 13, 36, 52), (3, 5, 12, 20), (1, 7, 4, 28),
           (16, 16, 16, 16), (16, 24, 8, 12), (16, 16, 5, 5), (17, 17, 68, 68)]


# ---- an exact fp32 run passes with half of every bound ------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,classes,ld', CE_SHAPES)
def test_ce_fp32_run_stays_inside_half_of_every_bound(rows, classes, ld):
    for s in (0.0, 0.1, 1.0):
        for ign in (-100, 255):
            z, t = L.make_ce(rows, classes, ign, seed=rows + classes)
            ref = L.CERef(z, t, ign, s)
            l, rl, loss, den = L.ce_fp32(z, t, ign, s)
            L.check_ce_fwd('fp32', ref, l, rl, frac=0.5)
            L.check_ce_mean('fp32', ref, loss, rl)
            d = L.ce_fp32_bwd(z, t, ign, s, ref.lse32, den, 0.7)
            L.check_ce_bwd('fp32', ref, 0.7, d, frac=0.5)
            L.check_ce_bwd('bf16', ref, 0.7, d.to(BF))                   # and, rounded once, the whole bound


@pytest.mark.parametrize('hs,ws,hd,wd', UP_GEOM)
def test_upsample_ce_fp32_run_stays_inside_half_of_every_bound(hs, ws, hd, wd):
    n = 3 if hs == 17 else 2
    for classes in (3, 19):
        low, t = L.make_up(n, hs, ws, classes, hd, wd, seed=hs + wd + classes)
        ref = L.UpRef(low, t, hd, wd, 255, gs=1.3)
        up, l, rl, loss, den, axes = L.up_fp32(low, t, hd, wd, 255)
        L.check_ce_fwd('fp32', ref.ce, l, rl, frac=0.5)
        dlow = L.up_fp32_bwd(up, t, ref.shape, 255, ref.ce.lse32, den, 1.3, axes)
        ref.check_bwd('fp32', dlow, frac=0.5)
        prev = torch.randn(dlow.shape).to(BF)
        ref.check_bwd('fp32', dlow + prev.float(), prev=prev, frac=0.5)
        assert bool((ref.dlow[:, ref.unmapped] == 0).all())


def test_upsample_ce_dyadic_case_takes_no_slack():
    low, t = L.make_up(2, 8, 8, 19, 32, 32, seed=5, dyadic=True)
    ref = L.UpRef(low, t, 32, 32, 255, exact=True)
    assert ref.n_slack == 0
    up, l, rl, loss, den, axes = L.up_fp32(low, t, 32, 32, 255)
    assert torch.equal(up.double(), ref.up), 'the exact interpolant rounds to the same bf16 values'
    L.check_ce_fwd('fp32', ref.ce, l, rl, frac=0.5)
    with pytest.raises(AssertionError):                                   # random inputs are not an exact case
        L.UpRef(L.make_up(1, 8, 8, 3, 33, 33, seed=5)[0], t[:1, :, :], 33, 33, 255, exact=True)


@pytest.mark.parametrize('mode,rows,classes', [(0, 777, 5), (0, 5000, 19), (0, 8193, 64), (0, 8192, 63), (1, 4099, 1), (2, 777, 5),
                                                (2, 5000, 19)])
def test_dice_fp32_run_stays_inside_half_of_every_bound(mode, rows, classes):
    empty = 1 if classes > 2 else None
    z, t = L.make_dice(rows, classes, mode, seed=rows, empty_class=empty)
    for log_loss in (0, 1):
        for smooth in (0.0, 1.0):
            for sel in (None, [0, 1, classes - 1] if classes > 2 else None):
                ref = L.DiceRef(z, t, mode, L.dice_rows(rows))
                I, Pp, Y, loss, coef, d = L.dice_fp32(z, t, mode, smooth, 1e-7, log_loss, sel, 0.9)
                assert torch.equal(Y.double(), ref.Y)
                assert_bounded(I, ref.I, ref.m_I, 0.0, 0.5 * U32, 'I')
                assert_bounded(Pp, ref.P, ref.m_P, 0.0, 0.5 * U32, 'P')
                # finalize alone: the fp64 formula on the sums the fp32 run produced
                l64, m_l, c64 = ref.finalize(I.double(), Pp.double(), Y.double(), smooth, 1e-7, log_loss, sel)
                assert_bounded(loss.reshape(1), l64.reshape(1), m_l.reshape(1), 0.0, 0.5 * U32, 'loss')
                assert_bounded(coef, c64, c64.abs(), 0.0, 0.5 * ref.K_FIN * U32, 'coef')
                if empty is not None:
                    assert float(coef[0, empty]) == 0 and float(coef[1, empty]) == 0
                # backward alone (its own coef), then end to end
                w, mag = ref.grad(coef.double(), 0.9)
                assert_bounded(d, w, mag, 0.0, 0.5 * U32, 'dlogits of its own coef')
                l64, m_l, c64 = ref.finalize(ref.I, ref.P, ref.Y, smooth, 1e-7, log_loss, sel)
                w, mag = ref.grad(c64, 0.9, ref.coef_rel(0.5))
                assert_bounded(d, w, mag, 0.0, 0.5 * U32, 'dlogits end to end')


@pytest.mark.parametrize('rows,classes,mean', [(37, 21, 1), (5, 1, 0), (1171, 7, 1), (3001, 16, 0)])
def test_bce_fp32_run_stays_inside_half_of_every_bound(rows, classes, mean):
    z, t = L.make_bce(rows, classes, -1.0, seed=rows)
    loss64, b_loss, n, d64, mag = L.bce_ref(z, t, -1.0, mean, 1.7)
    loss, d = L.bce_fp32(z, t, -1.0, mean, 1.7)
    assert_bounded(loss.reshape(1), loss64.reshape(1), b_loss.reshape(1), 0.0, 0.5, 'loss')
    assert_bounded(d, d64, mag, 0.0, 0.5 * U32, 'dlogits')
    # everything ignored: loss 0, gradient 0
    t[:] = -1.0
    loss64, b_loss, n, d64, mag = L.bce_ref(z, t, -1.0, mean, 1.7)
    assert n == 0 and float(loss64) == 0 and float(d64.abs().max()) == 0


@pytest.mark.parametrize('n', [1, 8191, 8193, 70001])
def test_regression_fp32_run_stays_inside_half_of_every_bound(n):
    for kind in range(4):
        for knee in (0.5, 1.5):
            for mean in (0, 1):
                x, t = L.make_reg(n, knee, seed=n + kind)
                loss64, b_loss, d64, mag = L.reg_ref(x, t, kind, knee, mean, 1.3)
                loss, d = L.reg_fp32(x, t, kind, knee, mean, 1.3)
                assert_bounded(loss.reshape(1), loss64.reshape(1), b_loss.reshape(1), 0.0, 0.5, 'loss')
                assert_bounded(d, d64, mag, 0.0, 0.5 * U32, 'dx')
                if kind == 3 and n > 8:
                    with pytest.raises(AssertionError):
                        assert_bounded(L.reg_fp32(x, t, kind, knee, mean, 1.3, wrong='huber_unit_slope')[1].to(BF), d64, mag, A_BF, U32)


# ---- wrong variants do not pass -----------------------------------------------------------------------------------------------------
def test_wrong_fp32_variants_are_rejected():
    rows, classes, ld = 37, 65, 72
    z, t = L.make_ce(rows, classes, -100, seed=3)
    ref = L.CERef(z, t, -100, 0.1)
    l, rl, loss, den = L.ce_fp32(z, t, -100, 0.1)
    with pytest.raises(AssertionError):                          # s / ld in place of s / classes
        L.check_ce_bwd('wrong', ref, 1.0, L.ce_fp32_bwd(z, t, -100, 0.1, ref.lse32, den, 1.0, wrong='s_over_ld', ld=ld).to(BF))
    l, rl, loss, den = L.ce_fp32(z, t, -100, 0.0, wrong='mean_all_rows')
    with pytest.raises(AssertionError):                          # the mean over all rows (s = 0: the -inf row keeps a finite loss)
        L.check_ce_mean('wrong', L.CERef(z, t, -100, 0.0), loss, rl)
    with pytest.raises(AssertionError):                          # ... and its gradient, scaled by 1 / rows
        L.check_ce_bwd('wrong', ref, 1.0, L.ce_fp32_bwd(z, t, -100, 0.1, ref.lse32, den, 1.0).to(BF))
    low, tu = L.make_up(2, 8, 8, 19, 33, 33, seed=4)
    uref = L.UpRef(low, tu, 33, 33, 255)
    up, l, rl, loss, den, axes = L.up_fp32(low, tu, 33, 33, 255, wrong='swap_y')
    with pytest.raises(AssertionError):                          # the weights of y0 and y1 exchanged
        L.check_ce_fwd('wrong', uref.ce, l, rl)
    up, l, rl, loss, den, good = L.up_fp32(low, tu, 33, 33, 255)
    with pytest.raises(AssertionError):                          # ... in the adjoint only
        uref.check_bwd('wrong', L.up_fp32_bwd(up, tu, uref.shape, 255, uref.ce.lse32, den, 1.0, axes).to(BF))


# ---- the references against torch and the fake backend --------------------------------------------------------------------------------
def test_ce_reference_agrees_with_torch_and_the_fake_backend():
    rows, classes, ld = 37, 19, 24
    for s in (0.0, 0.1, 1.0):
        z, t = L.make_ce(rows, classes, -100, seed=1)
        z[6, classes - 1] = -3.0                                   # (keep the smoothed loss finite for the comparison)
        ref = L.CERef(z, t, -100, s)
        zz = z.double().requires_grad_(True)
        tt = torch.where(ref.valid, t, torch.full_like(t, -100))   # torch raises on labels it does not know: dropped here
        loss = F.cross_entropy(zz, tt, ignore_index=-100, label_smoothing=s)
        loss.backward()
        assert abs(float(ref.row_loss.sum() / ref.n_valid) - float(loss)) < 1e-12 * max(1.0, abs(float(loss)))
        assert (F.cross_entropy(zz, tt, ignore_index=-100, label_smoothing=s, reduction='none').detach() - ref.row_loss).abs().max() < 1e-10
        d, _, _ = ref.grad(1.0)
        assert (d - zz.grad).abs().max() < 1e-6                    # (ref: the fp32-rounded lse)
        fake = FakeTok()
        buf = torch.zeros(rows, ld, dtype=BF)
        buf[:, :classes] = z
        lse, rl, lo, dl = torch.empty(rows), torch.empty(rows), torch.zeros(2), torch.empty(rows, ld, dtype=BF)
        gs = torch.tensor([0.7])
        assert fake.tok_softmax_ce_smooth_fwd(P(buf), P(t), rows, classes, ld, -100, s, P(lse), P(rl), P(lo), None) == 0
        L.check_ce_fwd('fake', ref, lse, rl)
        L.check_ce_mean('fake', ref, lo, rl)
        assert fake.tok_softmax_ce_smooth_bwd(P(buf), P(t), P(ref.lse32), P(lo), P(gs), rows, classes, ld, -100, s, P(dl), None) == 0
        L.check_ce_bwd('fake', ref, 0.7, dl[:, :classes])
        assert bool((dl[:, classes:] == 0).all())


def test_upsample_reference_agrees_with_interpolate_then_cross_entropy():
    n, hs, ws, classes, hd, wd = 2, 9, 13, 19, 36, 52
    low, t = L.make_up(n, hs, ws, classes, hd, wd, seed=2)
    ref = L.UpRef(low, t, hd, wd, 255)
    up = F.interpolate(low.double().permute(0, 3, 1, 2), size=(hd, wd), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    assert (up - ref.v).abs().max() < 1e-5                         # (ref: ATen's fp32 indices and weights)
    up32 = F.interpolate(low.float().permute(0, 3, 1, 2), size=(hd, wd), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    differs = up32.to(BF).reshape(-1, classes).double() != ref.up
    assert int((differs & (ref.ce.slack == 0)).sum()) == 0, 'ATen rounds to another bf16 value outside the tie set'
    # the adjoint against autograd, on the reference's own bf16(d upsampled logits)
    x = low.double().permute(0, 3, 1, 2).requires_grad_(True)
    y = F.interpolate(x, size=(hd, wd), mode='bilinear', align_corners=False)
    y.backward(ref.dup.reshape(n, hd, wd, classes).permute(0, 3, 1, 2))
    assert (x.grad.permute(0, 2, 3, 1) - ref.dlow).abs().max() < 1e-6 * max(1.0, float(ref.dlow.abs().max()))
    fake = FakeTok()
    ld = 24
    buf = torch.zeros(n, hs, ws, ld, dtype=BF)
    buf[..., :classes] = low
    rows = n * hd * wd
    lse, rl, lo, dl = torch.empty(rows), torch.empty(rows), torch.zeros(2), torch.full((n, hs, ws, ld), 9.0, dtype=BF)
    assert fake.tok_upsample_ce_fwd(P(buf), n, hs, ws, classes, ld, hd, wd, P(t), 255, P(lse), P(rl), P(lo), None) == 0
    L.check_ce_fwd('fake', ref.ce, lse, rl)
    L.check_ce_mean('fake', ref.ce, lo, rl)
    assert fake.tok_upsample_ce_bwd(P(buf), n, hs, ws, classes, ld, hd, wd, P(t), 255, P(ref.ce.lse32), P(lo), None, P(dl), 0, None) == 0
    ref.check_bwd('fake', dl[..., :classes])
    assert bool((dl[..., classes:] == 0).all())
    assert L.up_tiled_ok(8, 8, 32, 32) and not L.up_tiled_ok(8, 8, 33, 33) and not L.up_tiled_ok(8, 4, 16, 32)


def test_bce_and_regression_references_agree_with_torch_and_the_fake_backend():
    z, t = L.make_bce(37, 21, -1.0, seed=3)
    sel = t != -1.0
    for mean in (0, 1):
        loss64, b_loss, n, d64, mag = L.bce_ref(z, t, -1.0, mean, 1.0)
        x = z.double().requires_grad_(True)
        want = F.binary_cross_entropy_with_logits(x[sel], t.double()[sel], reduction='mean' if mean else 'sum')
        want.backward()
        assert abs(float(want) - float(loss64)) < 1e-12 * abs(float(want)) and (x.grad - d64).abs().max() < 1e-14
        fake, lo, dl, gs = FakeTok(), torch.zeros(2), torch.empty(37, 24, dtype=BF), torch.tensor([1.0])
        buf = torch.zeros(37, 24, dtype=BF)
        buf[:, :21] = z
        assert fake.tok_bce_logits_fwd(P(buf), P(t), 37, 21, 24, -1.0, mean, P(lo), None) == 0
        assert_bounded(lo[0:1], loss64.reshape(1), b_loss.reshape(1), 0.0, 1.0, 'fake loss')
        assert float(lo[1]) == n
        assert fake.tok_bce_logits_bwd(P(buf), P(t), P(lo), P(gs), 37, 21, 24, -1.0, mean, P(dl), None) == 0
        assert_bounded(dl[:, :21], d64, mag, A_BF, U32, 'fake dlogits')
    fns = {0: lambda a, b, k: F.l1_loss(a, b, reduction='none'), 1: lambda a, b, k: F.mse_loss(a, b, reduction='none'),
           2: lambda a, b, k: F.smooth_l1_loss(a, b, reduction='none', beta=k), 3: lambda a, b, k: F.huber_loss(a, b, reduction='none', delta=k)}
    for kind in range(4):
        for knee in (0.5, 1.5):
            xb, tt = L.make_reg(8193, knee, seed=kind)
            loss64, b_loss, d64, mag = L.reg_ref(xb, tt, kind, knee, 1, 1.0)
            x = xb.double().requires_grad_(True)
            want = fns[kind](x, tt.double(), knee).mean()
            want.backward()
            assert abs(float(want) - float(loss64)) < 1e-12 * abs(float(want))
            # torch's subgradient of |d| at 0 is 0 as well; at the knee both branches have the same slope
            assert (x.grad - d64).abs().max() < 1e-15
            fake, lo, dx, gs = FakeTok(), torch.zeros(2), torch.empty(8193, dtype=BF), torch.tensor([1.0])
            assert fake.tok_regression_loss_fwd(P(xb), P(tt), 8193, kind, knee, 1, P(lo), None) == 0
            assert_bounded(lo[0:1], loss64.reshape(1), b_loss.reshape(1), 0.0, 1.0, 'fake loss')
            assert fake.tok_regression_loss_bwd(P(xb), P(tt), P(gs), 8193, kind, knee, 1, P(dx), None) == 0
            assert_bounded(dx, d64, mag, A_BF, U32, 'fake dx')


def test_dice_and_count_references_agree_with_the_fake_backend():
    rows, classes, ld = 777, 5, 8
    for mode in (0, 2):
        z, t = L.make_dice(rows, classes, mode, seed=4, empty_class=1)
        ref = L.DiceRef(z, t, mode, L.dice_rows(rows))
        sel = torch.tensor([0, 1, 4])
        l64, m_l, c64 = ref.finalize(ref.I, ref.P, ref.Y, 1.0, 1e-7, 1, [0, 1, 4])
        fake = FakeTok()
        buf = torch.zeros(rows, ld, dtype=BF)
        buf[:, :classes] = z
        part, lo, co, dl = torch.zeros(1, 3, classes), torch.zeros(1), torch.zeros(2, classes), torch.empty(rows, ld, dtype=BF)
        assert fake.tok_dice_fwd(P(buf), P(t), rows, classes, ld, mode, 1.0, 1e-7, 1, P(sel), 3, P(part), P(lo), P(co), None) == 0
        assert abs(float(lo[0]) - float(l64)) < 1e-5 and (co.double() - c64).abs().max() < 1e-5 * c64.abs().max()
        assert fake.tok_dice_bwd(P(buf), P(t), P(co), None, rows, classes, ld, mode, P(dl), None) == 0
        w, mag = ref.grad(co.double(), 1.0)
        assert_bounded(dl[:, :classes], w, mag, A_BF, U32, 'fake dlogits')
    assert [L.dice_rows(r) for r in (1, 4, 5, 8192, 8193, 100003)] == [1, 1, 2, 2048, 2048, 2048]
    for classes in (1, 3, 70):
        z, lab, t = L.make_counts(200, classes, 255, seed=classes)
        buf = torch.zeros(200, classes, dtype=BF)
        buf.copy_(z)
        for pred, args in ((z, (P(buf), None)), (lab, (None, P(lab)))):
            counts, conf = L.counts_ref(pred, t, classes, 255)
            c1, c2 = torch.ones(3, classes, dtype=torch.int64), torch.ones(classes, classes, dtype=torch.int64)
            fake = FakeTok()
            assert fake.tok_cls_stats_update(*args, P(t), 200, classes, classes, 255, P(c1), None) == 0
            assert fake.tok_confusion_update(*args, P(t), 200, classes, classes, 255, P(c2), None) == 0
            assert torch.equal(c1 - 1, counts) and torch.equal(c2 - 1, conf)
    z = torch.full((3, 4), -math.inf).to(BF)
    counts, conf = L.counts_ref(z, torch.tensor([0, 1, 3]), 4, 255)
    assert counts.tolist() == [[1, 0, 0, 0], [3, 0, 0, 0], [1, 1, 0, 1]]
