"""tok_upsample_dice_fwd / _bwd (multiclass Dice on bilinearly upsampled logits, from the low-resolution logits) against fp64, the
public route through SegmentationHead + DiceLoss, and the fallbacks and refusals.

Reference: interpolation in fp64 by the source-index rule of tests/resample_ref.py, rounded to bf16 as the head's stored output
would be; softmax, Dice (loss_ref.DiceRef.finalize's definition) and autograd in fp64; the adjoint of the interpolation by
resample_ref.up64_T.  Tolerances are those of tests/test_dice.py: loss 2e-3 relative + 1e-5, gradient rel_err < 1e-2 (bf16 storage).
Every case carries a class without a true pixel (class 1) and three rows of labels 255 (outside the classes: they add to P only)."""
import pytest
import torch

from helpers import A_BF, ERR_INVALID, F32, GuardedSpan, Mat, cdiv, rel_err
import loss_ref as L
import resample_ref as RR
import torchok_amd as T
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr
from torchok_amd.losses import cross_entropy as CE
from torchok_amd.losses.base import JointLoss

pytestmark = pytest.mark.gpu
P = lambda t: None if t is None else t.data_ptr()       # noqa: E731
BITS = lambda q: q.contiguous().view(torch.int16 if q.dtype == torch.bfloat16 else torch.int32)        # noqa: E731
GS = 1.3


def _data(n, hs, ws, classes, hd, wd):
    g = torch.Generator().manual_seed(hs + wd + classes)
    low = L.bf(torch.randn(n, hs, ws, classes, generator=g) * 2)
    t = torch.randint(0, classes, (n, hd, wd), generator=g)
    t[t == 1] = 0
    t[:, :3] = 255
    return low, t


def _ref(low, t, size, smooth=0.0, eps=1e-7, log_loss=False, sel=None):
    """fp64 loss and GS * d loss / d low"""
    c = low.shape[-1]
    up = L.bf(RR.up64(low, size).float()).double().requires_grad_(True)
    p = up.softmax(-1)
    y = (t[..., None] == torch.arange(c)).double()
    i, ps, ys = (p * y).sum((0, 1, 2)), p.sum((0, 1, 2)), y.sum((0, 1, 2))
    score = (2 * i + smooth) / ((ps + ys).clamp_min(eps) + smooth)
    per = (-torch.log(score.clamp_min(eps)) if log_loss else 1 - score) * (ys > 0)
    loss = (per if sel is None else per[sel]).mean()
    (GS * loss).backward()
    return float(loss.detach()), RR.up64_T(up.grad, low.shape[1:3])


def _pair(classes, ld, hs, ws, hd, wd, form, **kw):
    lib, st, n = _C.lib(), stream_ptr(), 2
    assert lib.tok_upsample_dice_serves(classes, ld) == 1 and ('tiled' if L.up_tiled_ok(hs, ws, hd, wd) else 'gather') == form
    low, t = _data(n, hs, ws, classes, hd, wd)
    want_loss, want_d = _ref(low, t, (hd, wd), **kw)
    rows, tc = lib.tok_upsample_dice_rows(n, hd, wd), t.cuda()
    assert rows == min(n * cdiv(hd, 16) * cdiv(wd, 16), 1024)
    sel = None if kw.get('sel') is None else torch.tensor(kw['sel'], device='cuda')
    zg = Mat(n * hs * ws, classes, ld, init=low.cuda(), nan=True)
    prev = L.bf(torch.randn(n * hs * ws, ld, generator=torch.Generator().manual_seed(1)))
    gs, runs = torch.tensor([GS], device='cuda'), []
    for _ in range(2):
        lg, pg, lo, cg = Mat(1, n * hd * wd, dtype=F32), Mat(rows, 3 * classes, dtype=F32), GuardedSpan(1, F32, 64), Mat(2, classes, dtype=F32)
        _C.check(lib.tok_upsample_dice_fwd(zg.ptr, n, hs, ws, classes, ld, hd, wd, P(tc), kw.get('smooth', 0.0), 1e-7,
                                           int(kw.get('log_loss', False)), P(sel), 0 if sel is None else sel.numel(), lg.ptr, pg.ptr,
                                           lo.ptr, cg.ptr, st), 'fwd')
        d = [Mat(n * hs * ws, classes, ld), Mat(n * hs * ws, classes, ld, init=prev[:, :classes].cuda())]
        d[1].full[:, classes:] = prev[:, classes:].cuda()
        for acc in (0, 1):
            _C.check(lib.tok_upsample_dice_bwd(zg.ptr, n, hs, ws, classes, ld, hd, wd, P(tc), lg.ptr, cg.ptr, P(gs), d[acc].ptr, acc, st), 'bwd')
        torch.cuda.synchronize()
        runs.append([lg, pg, cg, d[0], d[1], lo])
    lg, pg, cg, d0, d1, lo = runs[0]
    for m, what in ((lg, 'lse'), (pg, 'partial'), (cg, 'coef')):
        m.done(what)
    zg.done('low', finite=False)
    lo.check('loss')
    d0.done('dlow', zero_pads=True)             # every owned element written over the sentinel, columns [classes, ld) exactly zero
    d1.span.check('dlow +=')
    whole = lambda m: BITS(m.view if isinstance(m, GuardedSpan) else m.full)        # noqa: E731
    assert all(torch.equal(whole(a), whole(b)) for a, b in zip(*runs)), 'two runs differ'
    got = float(lo.value()[0])
    print(f'loss {got:.7f} want {want_loss:.7f}  dlow rel_err {rel_err(d0.value().float(), want_d.reshape(-1, classes)):.2e}')
    assert abs(got - want_loss) < 2e-3 * abs(want_loss) + 1e-5
    assert rel_err(d0.value().float(), want_d.reshape(-1, classes)) < 1e-2
    assert torch.equal(cg.value()[:, 1], torch.zeros(2))                        # the class without a true pixel
    # += is = plus the previous value, the sum rounded once more
    both = d0.full.float().cpu() + prev.float()
    assert bool(((d1.full.float().cpu() - both).abs() <= A_BF * torch.maximum(both.abs(), d0.full.float().cpu().abs())).all())


WIDTHS = [(3, 8), (19, 24), (33, 40), (64, 64)]     # one lane a pixel; dead lanes in a group of 4 and of 8; a full group of 8
GEOM = [(16, 24, 64, 96, 'tiled'),                  # scale 4
        (7, 5, 30, 17, 'gather'),                   # non-integer scale past 4, ragged tiles on both sides, clamped borders
        (9, 9, 9, 9, 'tiled'),                      # identity
        (12, 12, 5, 7, 'tiled'),                    # downsampling; at ld = 64 the footprint leaves LDS: taps from global memory
        (4, 4, 32, 32, 'gather')]                   # scale 8


@pytest.mark.parametrize('classes,ld,hs,ws,hd,wd,form', [w + g for w in WIDTHS for g in GEOM] +
                         [(3, 8, 92, 92, 368, 368, 'tiled')])      # 2 x 23 x 23 tiles: more than the 1024 partial rows
def test_kernel_pair(classes, ld, hs, ws, hd, wd, form):
    _pair(classes, ld, hs, ws, hd, wd, form)


@pytest.mark.parametrize('kw', [dict(log_loss=True, smooth=1.0), dict(sel=[0, 2])])
def test_kernel_pair_options(kw):
    _pair(19, 24, 16, 24, 64, 96, 'tiled', **kw)


@pytest.mark.parametrize('losses', ['ce+dice', 'dice'])
def test_head_losses_run_on_the_low_resolution_logits(losses, monkeypatch):
    """SegmentationHead(32, 19) on 16x24 features of a 64x96 image: nothing is materialised, and loss and gradients are those of
    the materialised route (FUSE_UPSAMPLE_CE off) within the tolerances of test_dice.py's lazy-logits test."""
    img = torch.zeros(2, 3, 64, 96, device='cuda')
    x = torch.randn(2, 32, 16, 24, generator=torch.Generator().manual_seed(2)).cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, 19, (2, 64, 96), generator=torch.Generator().manual_seed(3)).cuda()

    def run(lazy):
        monkeypatch.setattr(CE, 'FUSE_UPSAMPLE_CE', lazy)
        torch.manual_seed(0)
        head = T.HEADS.get('SegmentationHead')(in_channels=32, num_classes=19).cuda().train()
        mods = [T.LOSSES.get('CrossEntropyLoss')()] * (losses == 'ce+dice') + [T.LOSSES.get('DiceLoss')('multiclass')]
        joint = JointLoss(mods, [{'input': 'prediction', 'target': 'target'}] * len(mods), [None] * len(mods), [None] * len(mods))
        feat = x.clone().requires_grad_(True)
        out = head([img, feat])
        loss, _ = joint(prediction=out, target=t)
        loss.backward()
        assert not lazy or (isinstance(out, CE.UpsampledLogits) and out._full is None)
        return float(loss.detach()), [feat.grad.float(), head.classifier.weight.grad.float(), head.classifier.bias.grad.float()]
    l0, g0 = run(False)
    l1, g1 = run(True)
    assert abs(l0 - l1) < 2e-3 * max(1.0, abs(l0))
    for a, b in zip(g1, g0):
        assert float(a.abs().max()) > 0 and rel_err(a, b) < 2e-2, rel_err(a, b)


@pytest.mark.parametrize('mode,classes,full', [('multilabel', 5, False), ('binary', 5, False), ('multiclass', 65, False),
                                               ('multiclass', 19, True)])
def test_fallbacks_materialise(mode, classes, full):
    """what the fused kernels do not serve takes today's route: the interpolated tensor exists afterwards and the loss is the
    unfused one's on it, bit for bit ('binary' takes every element of the 5-channel output as a logit of its own)"""
    torch.manual_seed(classes)
    head = T.HEADS.get('SegmentationHead')(in_channels=32, num_classes=classes).cuda().train()
    feat = torch.randn(2, 32, 4, 4, device='cuda').to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    u = head([torch.zeros(2, 3, 16, 16, device='cuda'), feat])
    assert isinstance(u, CE.UpsampledLogits) and u._full is None
    if full:
        u.materialize()
    t = torch.randint(0, classes, (2, 16, 16), device='cuda') if mode == 'multiclass' else (torch.rand(2, classes, 16, 16, device='cuda') < 0.4).float()
    dice = T.LOSSES.get('DiceLoss')(mode, smooth=0.5)
    if classes > 64:                              # tok_dice_fwd's own limit: refused, as before, on the materialised tensor
        with pytest.raises(_C.TokError, match='tok_dice_fwd'):
            dice(u, t)
        assert u._full is not None
        return
    loss = dice(u, t)
    loss.backward()
    assert u._full is not None and float(feat.grad.abs().max()) > 0
    assert float(loss.detach()) == float(dice(u._full.detach(), t))


def test_wrong_target_size_raises():
    u = CE.UpsampledLogits(torch.zeros(2, 19, 4, 4, device='cuda', dtype=torch.bfloat16), (16, 16))
    with pytest.raises(ValueError):
        T.LOSSES.get('DiceLoss')('multiclass')(u, torch.zeros(2, 15, 16, dtype=torch.int64, device='cuda'))


@pytest.mark.parametrize('classes,ld,off,null', [(9, 12, 0, False), (65, 72, 0, False), (19, 24, 4, False), (19, 24, 0, True)])
def test_refusals(classes, ld, off, null):
    """ld % 8 != 0, ld > 64, low not 16-byte aligned, a null pointer: TOK_ERR_INVALID, nothing written"""
    lib, st, (n, hs, ws, hd, wd) = _C.lib(), stream_ptr(), (1, 4, 4, 8, 8)
    assert lib.tok_upsample_dice_serves(classes, ld) == (1 if off or null else 0) and lib.tok_upsample_dice_rows(0, hd, wd) == ERR_INVALID
    zg = Mat(n * hs * ws, ld, ld, init=torch.zeros(n * hs * ws, ld).cuda(), nan=True, off=off)
    t = torch.zeros(n, hd, wd, dtype=torch.int64, device='cuda')
    lg, pg, lo, cg, dg = Mat(1, n * hd * wd, dtype=F32), Mat(1, 3 * classes, dtype=F32), GuardedSpan(1, F32, 64), Mat(2, classes, dtype=F32), Mat(n * hs * ws, ld, ld)
    l32, c32 = torch.zeros(n * hd * wd, device='cuda'), torch.zeros(2, classes, device='cuda')
    low = None if null else zg.ptr
    assert lib.tok_upsample_dice_fwd(low, n, hs, ws, classes, ld, hd, wd, P(t), 0.0, 1e-7, 0, None, 0, lg.ptr, pg.ptr, lo.ptr, cg.ptr, st) == ERR_INVALID
    assert lib.tok_upsample_dice_bwd(low, n, hs, ws, classes, ld, hd, wd, P(t), P(l32), P(c32), None, dg.ptr, 0, st) == ERR_INVALID
    torch.cuda.synchronize()
    for m, what in ((lg, 'lse'), (pg, 'partial'), (cg, 'coef'), (dg, 'dlow')):
        m.intact(what)
    assert lo.untouched()
