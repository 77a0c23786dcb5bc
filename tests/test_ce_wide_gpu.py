"""tok_upsample_ce_wide_* (rows of up to 256 classes, class weights) and tok_softmax_ce_weighted_* element by element against the
fp64 references of tests/loss_ref.py, with their bounds.  Class weights enter the references as follows, w_r = w[target of row r]:
  row_loss   w_r times the unweighted one; its bound scales with w_r (the product is one of the six operations the bound counts:
             without smoothing the kernels use two)
  loss[1]    the fp64 sum W of w_r over the valid rows, one fp32 rounding; loss[0] = (fp64 sum of the kernel's own row losses) / W
  gradient   the unweighted reference evaluated with the per-row scale gs w_r n_valid / W in place of gs (it divides by n_valid):
             the kernels' extra product and the rounding of loss[1] bring the chain p - onehot, g / loss[1], g w_r, the product to
             five roundings, inside the six that CERef.grad counts
The sum of exponentials of the wide forward is sequential inside a block of 32 classes and a butterfly of at most three steps
over the blocks: never longer than the ld sequential additions UpRef counts."""
import pytest
import torch
import torch.nn.functional as F

from helpers import ERR_INVALID, F32, U32, GuardedSpan, Mat, rel_err
import loss_ref as L
import torchok_amd as T
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
P = lambda t: None if t is None else t.data_ptr()       # noqa: E731
BITS = lambda q: q.contiguous().view(torch.int16)        # noqa: E731
LOSS_FLOATS = 2050
GS = 1.3


def _weights(classes):
    """two orders of magnitude, one class of weight zero"""
    w = (10.0 ** torch.linspace(-1, 1, classes)).float()
    w[1 % classes] = 0.0
    return w


def _rows(t, classes, w):
    """w_r per row (0 on dropped rows), their sum W, and the per-row gradient scale that stands for GS (see above)"""
    if w is None:
        return None, None, GS
    valid = L.ce_valid(t.reshape(-1), 255, classes)
    wr = w.double()[t.reshape(-1).clamp(0, classes - 1)] * valid
    return wr, wr.sum(), (GS * wr * int(valid.sum()) / wr.sum())[:, None]


def _weighted(ce, wr):
    """the forward part of a CERef under row weights"""
    if wr is not None:
        ce.row_loss, ce.b_rl, ce.w_rl = ce.row_loss * wr, ce.b_rl * wr, ce.w_rl * wr
    return ce


def _check_mean(tag, ce, W, lo, own):
    if W is None:
        return L.check_ce_mean(tag, ce, lo, own)
    lo = lo.double().cpu()
    L.bounded(lo[1:2], W.reshape(1), W.reshape(1), U32, 0.0, 'loss[1]', tag)
    mean = (own.double().cpu()[ce.valid].sum() / W).reshape(1)
    L.bounded(lo[0:1], mean, mean.abs(), U32, 2.0 ** -40, 'loss[0] vs its own rows', tag)


GEOM = [(5, 7, 20, 28, 'tiled'), (5, 7, 17, 23, 'tiled'), (6, 6, 6, 6, 'tiled'), (2, 2, 40, 40, 'gather'), (24, 24, 6, 6, 'tiled')]


@pytest.mark.parametrize('hs,ws,hd,wd,kernel', GEOM)
@pytest.mark.parametrize('classes,ld', [(33, 40), (150, 152), (256, 256), (19, 24)])
def test_upsample_ce_wide(classes, ld, hs, ws, hd, wd, kernel):
    """(33, 40): one lane of the group partly masked; (150, 152): 32 lanes, 13 idle; (19, 24): the narrow width the weighted loss
    routes here.  Integer and fractional scale with partial tiles, identity, the gather backward (ratio 20), and a downsampling
    whose footprint leaves LDS at the two wide rows (taps from global memory)."""
    lib, st, n = _C.lib(), stream_ptr(), 2
    assert ('tiled' if L.up_tiled_ok(hs, ws, hd, wd) else 'gather') == kernel and lib.tok_upsample_ce_wide_serves(classes, ld) == 1
    low, t = L.make_up(n, hs, ws, classes, hd, wd, seed=hs + wd + classes)
    rows, tc = n * hd * wd, t.cuda()
    zg = Mat(n * hs * ws, classes, ld, init=low.cuda(), nan=True)
    prev = L.bf(torch.randn(n, hs, ws, ld, generator=torch.Generator().manual_seed(1)))
    for w in (None, _weights(classes)):
        tag = f'ce_wide/upce_{kernel}' + ('' if w is None else '_weighted')
        wc = None if w is None else w.cuda()
        wr, W, gsr = _rows(t, classes, w)
        ref = L.UpRef(low, t, hd, wd, 255, gs=gsr)
        _weighted(ref.ce, wr)
        runs = []
        for _ in range(2):
            lg, rg, lo = Mat(1, rows, dtype=F32), Mat(1, rows, dtype=F32), GuardedSpan(LOSS_FLOATS, F32, 64)
            _C.check(lib.tok_upsample_ce_wide_fwd(zg.ptr, n, hs, ws, classes, ld, hd, wd, P(tc), 255, P(wc), lg.ptr, rg.ptr, lo.ptr, st), 'fwd')
            out = [lg, rg, lo, None, None]
            for acc in (0, 1):
                dg = Mat(n * hs * ws, ld, ld, init=(prev if acc else torch.full((n, hs, ws, ld), 9.0)).cuda())
                _C.check(lib.tok_upsample_ce_wide_bwd(zg.ptr, n, hs, ws, classes, ld, hd, wd, P(tc), 255, P(wc), P(ref.ce.lse32.cuda()),
                                                      lo.ptr, P(torch.tensor([GS], device='cuda')), dg.ptr, acc, st), 'bwd')
                out[3 + acc] = dg
            torch.cuda.synchronize()
            runs.append(out)
        lg, rg, lo, d0, d1 = runs[0]
        zg.done('low')
        lg.done('lse')
        rg.done('row_loss')
        lo.check('loss')
        L.check_ce_fwd(tag, ref.ce, lg.view[0], rg.view[0])
        _check_mean(tag, ref.ce, W, lo.view[:2], rg.view[0])
        for acc, dg in ((0, d0), (1, d1)):
            dg.span.check('dlow')
            d = dg.value().view(n, hs, ws, ld)
            ref.check_bwd(tag, d[..., :classes], prev=prev[..., :classes] if acc else None)
            assert torch.equal(d[..., classes:], prev[..., classes:] if acc else torch.zeros_like(d[..., classes:])), 'pad channels'
        bits = [[BITS(m.view[:2] if m is r[2] else m.full) for m in r] for r in runs]
        assert all(torch.equal(a, b) for a, b in zip(*bits)), 'two runs differ'
        if w is None and ld <= 32:
            # without weights the wide entries are the narrow entries bit for bit
            nar = [Mat(1, rows, dtype=F32), Mat(1, rows, dtype=F32), GuardedSpan(LOSS_FLOATS, F32, 64), Mat(n * hs * ws, ld, ld)]
            _C.check(lib.tok_upsample_ce_fwd(zg.ptr, n, hs, ws, classes, ld, hd, wd, P(tc), 255, nar[0].ptr, nar[1].ptr, nar[2].ptr, st), 'narrow fwd')
            _C.check(lib.tok_upsample_ce_bwd(zg.ptr, n, hs, ws, classes, ld, hd, wd, P(tc), 255, P(ref.ce.lse32.cuda()), nar[2].ptr,
                                             P(torch.tensor([GS], device='cuda')), nar[3].ptr, 0, st), 'narrow bwd')
            torch.cuda.synchronize()
            assert all(torch.equal(BITS(m.view[:2] if m is nar[2] else m.full), b) for m, b in zip(nar, bits[0])), 'wide != narrow'


@pytest.mark.parametrize('classes,ld,off', [(260, 264, 0), (9, 12, 0), (33, 40, 4)])
def test_upsample_ce_wide_refusals(classes, ld, off):
    """ld > 256, ld % 8 != 0, low (or dlow) not 16-byte aligned: TOK_ERR_INVALID, nothing written"""
    lib, st, (n, hs, ws, hd, wd) = _C.lib(), stream_ptr(), (1, 4, 4, 8, 8)
    assert lib.tok_upsample_ce_wide_serves(classes, ld) == (1 if off else 0)
    zg = Mat(n * hs * ws, ld, ld, init=torch.zeros(n * hs * ws, ld).cuda(), nan=True, off=off)
    t = torch.zeros(n, hd, wd, dtype=torch.int64, device='cuda')
    lg, rg, lo = Mat(1, n * hd * wd, dtype=F32), Mat(1, n * hd * wd, dtype=F32), GuardedSpan(LOSS_FLOATS, F32, 64)
    dg, l32, l2 = Mat(n * hs * ws, ld, ld), torch.zeros(n * hd * wd, device='cuda'), torch.ones(LOSS_FLOATS, device='cuda')
    assert lib.tok_upsample_ce_wide_fwd(zg.ptr, n, hs, ws, classes, ld, hd, wd, P(t), 255, None, lg.ptr, rg.ptr, lo.ptr, st) == ERR_INVALID
    assert lib.tok_upsample_ce_wide_bwd(zg.ptr, n, hs, ws, classes, ld, hd, wd, P(t), 255, None, P(l32), P(l2), None, dg.ptr, 0, st) == ERR_INVALID
    torch.cuda.synchronize()
    for m, what in ((lg, 'lse'), (rg, 'row_loss'), (dg, 'dlow')):
        m.intact(what)
    assert lo.untouched()


@pytest.mark.parametrize('rows,classes,ld', [(37, 10, 10), (37, 10, 16), (5, 1000, 1000)])
def test_softmax_ce_weighted(rows, classes, ld):
    lib, st, tag = _C.lib(), stream_ptr(), 'ce_wide/ce_weighted'
    z, t = L.make_ce(rows, classes, 255, seed=rows + classes)
    w = _weights(classes)
    wr, W, gsr = _rows(t, classes, w)
    ref = _weighted(L.CERef(z, t, 255), wr)
    zg, tc, wc = Mat(rows, classes, ld, init=z.cuda(), nan=True), t.cuda(), w.cuda()
    lg, rg, lo, dg = Mat(1, rows, dtype=F32), Mat(1, rows, dtype=F32), GuardedSpan(LOSS_FLOATS, F32, 64), Mat(rows, classes, ld)
    _C.check(lib.tok_softmax_ce_weighted_fwd(zg.ptr, P(tc), P(wc), rows, classes, ld, 255, lg.ptr, rg.ptr, lo.ptr, st), 'fwd')
    _C.check(lib.tok_softmax_ce_weighted_bwd(zg.ptr, P(tc), P(wc), P(ref.lse32.cuda()), lo.ptr, P(torch.tensor([GS], device='cuda')),
                                             rows, classes, ld, 255, dg.ptr, st), 'bwd')
    torch.cuda.synchronize()
    zg.done('logits', finite=False)
    lg.done('lse')
    rg.done('row_loss')
    lo.check('loss')
    dg.done('dlogits', zero_pads=True)
    L.check_ce_fwd(tag, ref, lg.view[0], rg.view[0])
    _check_mean(tag, ref, W, lo.view[:2], rg.view[0])
    L.check_ce_bwd(tag, ref, gsr, dg.view)
    # and the loss against torch's own weighted mean in fp64: the row bounds, folded, and one rounding
    v = ref.valid
    want = F.cross_entropy(z.double()[v], t[v], weight=w.double()).reshape(1)
    L.bounded(lo.view[:1], want, (ref.b_rl.sum() / W + U32 * want.abs()).reshape(1), 0.0, 1.0, 'loss[0] vs torch', tag)


def test_weighted_loss_on_a_segmentation_head_stays_lazy():
    """CrossEntropyLoss(weight) on a SegmentationHead output with 40 classes runs on the low-resolution logits (nothing
    materialised); loss and low-resolution gradient against the fp64 reference by the rule of
    test_kernels_gpu.py::test_upsample_ce_equals_interpolate_then_cross_entropy (loss 1e-6 relative, gradient 1e-3)."""
    torch.manual_seed(0)
    classes = 40
    head = T.HEADS.get('SegmentationHead')(in_channels=32, num_classes=classes).cuda().train()
    img = torch.zeros(2, 3, 20, 28, device='cuda')
    feat = torch.randn(2, 32, 5, 7, device='cuda').to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, classes, (2, 20, 28), generator=torch.Generator().manual_seed(1))
    t[:, :3] = 255
    w = _weights(classes)
    out = head([img, feat.requires_grad_(True)])
    grads = []
    out._low.register_hook(grads.append)
    loss = T.LOSSES.get('CrossEntropyLoss')(weight=w, ignore_index=255).cuda()(input=out, target=t.cuda())
    loss.backward()
    assert out._full is None
    low = out._low.detach().permute(0, 2, 3, 1).cpu()
    wr, W, gsr = _rows(t, classes, w)
    ref = L.UpRef(low, t, 20, 28, 255, gs=gsr / GS)
    want = float((ref.ce.row_loss * wr).sum() / W)
    assert abs(float(loss.detach()) - want) <= 1e-6 * abs(want)
    # (the gradient is a bf16 tensor: the reference is rounded to bf16 like it, as both sides of that test are)
    assert rel_err(grads[0].permute(0, 2, 3, 1).float().cpu(), L.bf(ref.dlow.float()).float()) < 1e-3
