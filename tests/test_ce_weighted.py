"""CrossEntropyLoss with class weights and its route to the wide upsample-CE entries, on the host stand-in: construction,
the refusals that stay, and which native entries a lazy segmentation output with 40 classes reaches."""
import pytest
import torch
import torch.nn.functional as F

import fake_backend as fb
import torchok_amd as T
from torchok_amd.losses.cross_entropy import UpsampledLogits

BF = torch.bfloat16


class WideFake(fb.FakeTok):
    """FakeTok plus tok_softmax_ce_weighted_* and tok_upsample_ce_wide_* (the restatements of FakeTok, weighted)."""

    def tok_softmax_ce_weighted_fwd(self, logits, target, weight, rows, classes, ld, ignore_index, lse, row_loss, loss, st):
        rc = self.tok_softmax_ce_smooth_fwd(logits, target, rows, classes, ld, ignore_index, 0.0, lse, row_loss, loss, st)
        if weight is not None:
            t, rl = fb._t(target, (rows,), torch.int64), fb._t(row_loss, (rows,), torch.float32)
            wt = fb._t(weight, (classes,), torch.float32)[t.clamp(0, classes - 1)] * ((t != ignore_index) & (t >= 0) & (t < classes))
            rl.mul_(wt)
            o = fb._t(loss, (2,), torch.float32)
            o[1] = wt.double().sum().float()
            o[0] = (rl.double().sum() / wt.double().sum()).float()
        return rc

    def tok_softmax_ce_weighted_bwd(self, logits, target, weight, lse, loss, gscale, rows, classes, ld, ignore_index, dlogits, st):
        rc = self.tok_softmax_ce_smooth_bwd(logits, target, lse, loss, gscale, rows, classes, ld, ignore_index, 0.0, dlogits, st)
        if weight is not None:
            t, d = fb._t(target, (rows,), torch.int64), fb._t(dlogits, (rows, ld), BF)
            d.copy_(d.float() * fb._t(weight, (classes,), torch.float32)[t.clamp(0, classes - 1)][:, None])
        return rc

    def tok_upsample_ce_wide_serves(self, classes, ld):
        return int(0 < classes <= ld <= 256 and ld % 8 == 0)

    def tok_upsample_ce_wide_fwd(self, low, n, hs, ws, classes, ld, hd, wd, target, ignore_index, weight, lse, row_loss, loss, st):
        self.calls.append('upsample_ce_wide_fwd')
        up = self._upsampled(low, n, hs, ws, classes, ld, hd, wd)
        return self.tok_softmax_ce_weighted_fwd(up.data_ptr(), target, weight, n * hd * wd, classes, ld, ignore_index, lse,
                                                row_loss, loss, st)

    def tok_upsample_ce_wide_bwd(self, low, n, hs, ws, classes, ld, hd, wd, target, ignore_index, weight, lse, loss, gscale, dlow,
                                 accumulate, st):
        self.calls.append('upsample_ce_wide_bwd')
        up = self._upsampled(low, n, hs, ws, classes, ld, hd, wd)
        dup = torch.zeros(n * hd * wd, ld, dtype=BF)
        self.tok_softmax_ce_weighted_bwd(up.data_ptr(), target, weight, lse, loss, gscale, n * hd * wd, classes, ld, ignore_index,
                                         dup.data_ptr(), st)
        calls = list(self.calls)
        rc = self.tok_bilinear_bwd(dup.data_ptr(), n, hd, wd, ld, 0, dlow, hs, ws, classes, ld, accumulate, st)
        self.calls[:] = calls
        return rc


@pytest.fixture
def fake(request):
    token = fb.install(getattr(request, 'param', WideFake)())
    yield token[0]
    fb.uninstall(token)


def _case(classes, seed=0):
    g = torch.Generator().manual_seed(seed)
    low = (torch.randn(2, 5, 7, classes, generator=g) * 2).to(BF)        # channel-last, as a segmentation head leaves it
    t = torch.randint(0, classes, (2, 20, 28), generator=g)
    t[:, :2] = 255
    w = torch.rand(classes, generator=g) * 3 + 0.01
    w[1] = 0.0
    return low, t, w


@pytest.mark.parametrize('as_type', [torch.as_tensor, list, tuple])
def test_weight_is_accepted_and_kept_as_an_fp32_buffer(as_type):
    w = [0.5, 2.0, 0.0]
    m = T.LOSSES.get('CrossEntropyLoss')(weight=as_type(w))
    assert m.weight.dtype == torch.float32 and m.weight.tolist() == w and 'weight' in dict(m.named_buffers())
    assert 'weight' not in dict(T.LOSSES.get('CrossEntropyLoss')().named_buffers())


def test_refusals_that_stay():
    CE = T.LOSSES.get('CrossEntropyLoss')
    with pytest.raises(NotImplementedError, match='label_smoothing'):
        CE(weight=[1.0, 2.0], label_smoothing=0.1)
    for kw in (dict(reduction='none'), dict(size_average=True), dict(reduce=False)):
        with pytest.raises(NotImplementedError):
            CE(weight=[1.0, 2.0], **kw)


@pytest.mark.parametrize('lazy', [False, True])
def test_wrong_weight_length_raises(fake, lazy):
    low, t, w = _case(8)
    x = UpsampledLogits(low.permute(0, 3, 1, 2), (20, 28)) if lazy else low.permute(0, 3, 1, 2)
    with pytest.raises(ValueError, match='weight tensor should be defined either for all 8 classes'):
        T.LOSSES.get('CrossEntropyLoss')(weight=w[:5], ignore_index=255)(x, t if lazy else t[:, :5, :7])


WIDE, NARROW, PLAIN = ['upsample_ce_wide_fwd', 'upsample_ce_wide_bwd'], ['upsample_ce_fwd', 'upsample_ce_bwd'], ['bilinear_fwd', 'bilinear_bwd']


@pytest.mark.parametrize('fake,classes,weighted,want', [(WideFake, 40, False, WIDE), (WideFake, 40, True, WIDE), (WideFake, 19, True, WIDE),
                                                        (WideFake, 19, False, NARROW), (fb.FakeTok, 40, False, PLAIN),
                                                        (fb.FakeTok, 19, False, NARROW)], indirect=['fake'])
@pytest.mark.parametrize('reduction', ['mean', 'sum'])
def test_lazy_logits_route_and_value(fake, classes, weighted, want, reduction):
    """40 classes, or weights at any width, go to the wide entries and leave the input lazy; a backend without wide entries
    materialises as before; 19 classes without weights stay on the narrow entries.  Loss and gradient against torch in fp32."""
    low, t, w = _case(classes)
    low.requires_grad_(True)
    x = UpsampledLogits(low.permute(0, 3, 1, 2), (20, 28))
    loss = T.LOSSES.get('CrossEntropyLoss')(weight=w if weighted else None, ignore_index=255, reduction=reduction)(x, t)
    loss.backward()
    assert [c for c in fake.calls if 'upsample_ce' in c or 'bilinear' in c] == want
    assert (x._full is None) == (want[0] != 'bilinear_fwd')
    ref_low = low.detach().float().requires_grad_(True)
    up = F.interpolate(ref_low.permute(0, 3, 1, 2), size=(20, 28), mode='bilinear', align_corners=False)
    ref = F.cross_entropy(up, t, weight=w if weighted else None, ignore_index=255, reduction=reduction)
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) < 2e-2 * abs(float(ref.detach()))
    assert float((low.grad.float() - ref_low.grad).norm() / ref_low.grad.norm()) < 3e-2
