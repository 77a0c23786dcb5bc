"""Buffer lifetimes across streams in the no-grad / frozen forward (engine/core.py await_ready).

HRNet runs its branches and fuse rows on branch streams.  Fuse row i >= 1 reads x[0], which the main stream made; the
main stream joins the branch streams only in Region.output.  Without a tape node holding x[0] (no-grad, or a frozen
backbone whose input needs no gradient) its block went back to the main pool when the module returned, and the next
module's branch 0 could reuse it while rows 1-3 were still queued.  A tensor read on a stream other than the one it was
made on must be record_stream'ed there.  These tests run hrnet_w48 + neck + head at the product geometry three times
back-to-back with no synchronize in between and compare with the same forwards on the main stream alone, bit for bit.
A delay queued on each branch stream at entry widens the window in which a reused block would be overwritten."""
import pytest
import torch

import torchok_amd as T
from helpers import deterministic_state
from test_hrnet import seg_config
from torchok_amd.engine import core as EC
from torchok_amd.models.backbones import hrnet as HR

pytestmark = pytest.mark.gpu

SLEEP_CYCLES = 1_000_000       # torch.cuda._sleep: a bounded spin of ~0.5 ms per branch entry (the engine probes queues with it)


def _task():
    cfg = seg_config('hrnet_w48', classes=19, size=512)
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
    sd = deterministic_state({k: v for k, v in task.state_dict().items() if not k.startswith('input_tensors')}, 31)
    task.load_state_dict(sd, strict=False)
    return task.cuda()


def _inputs():
    g = torch.Generator().manual_seed(32)
    xs = [torch.randn(4, 3, 512, 1024, generator=g).cuda() for _ in range(3)]
    ys = [torch.randint(0, 19, (4, 512, 1024), generator=g).cuda() for _ in range(3)]
    return xs, ys


def _streams(monkeypatch, multi: bool):
    """multi: branch streams and fuse rows on them, with a delay queued on each branch stream at entry; otherwise every
    unit on the main stream."""
    monkeypatch.undo()
    monkeypatch.setattr(EC, 'BRANCH_STREAMS', multi)
    monkeypatch.setattr(HR, '_FUSE_STREAMS', multi)
    if multi:
        enter = EC._Branch.__enter__

        def delayed_enter(self):
            res = enter(self)
            if self.live:
                torch.cuda._sleep(SLEEP_CYCLES)
            return res
        monkeypatch.setattr(EC._Branch, '__enter__', delayed_enter)


def test_eval_no_grad_forwards_are_stream_transparent(monkeypatch):
    task = _task().eval()
    xs, _ = _inputs()
    res = {}
    for multi in (True, False):
        _streams(monkeypatch, multi)
        torch.cuda.synchronize()
        with torch.no_grad():
            outs = [task(x) for x in xs]          # three forwards, no synchronize between them
        torch.cuda.synchronize()
        res[multi] = [o.float().cpu() for o in outs]
    for i, (a, b) in enumerate(zip(res[True], res[False])):
        assert a.shape == (4, 19, 512, 1024) and torch.isfinite(a).all(), i
        assert torch.equal(a, b), (i, float((a - b).abs().max()))


def test_frozen_backbone_training_steps_are_stream_transparent(monkeypatch):
    """Frozen backbone (eval, no parameter needs a gradient: no tape in its region), neck and head training: three
    forward + backward passes back-to-back; losses and the accumulated neck / head gradients bit-identical."""
    xs, ys = _inputs()
    res = {}
    for multi in (True, False):
        _streams(monkeypatch, multi)
        task = _task().train()
        task.backbone.eval()
        for p in task.backbone.parameters():
            p.requires_grad_(False)
        torch.cuda.synchronize()
        losses = []
        for x, y in zip(xs, ys):
            out = task.forward_with_gt({'image': x, 'target': y})
            loss = task.losses(**out)[0]
            loss.backward()
            losses.append(loss.detach())
        torch.cuda.synchronize()
        res[multi] = ([float(v) for v in losses],
                      {n: p.grad.clone() for n, p in task.named_parameters() if p.requires_grad})
    assert res[True][0] == res[False][0]
    assert all(v == v for v in res[True][0])
    assert set(res[True][1]) == set(res[False][1]) and len(res[True][1]) > 0
    for n, g in res[True][1].items():
        assert torch.equal(g, res[False][1][n]), n
