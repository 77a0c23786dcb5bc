"""End-to-end parity (GPU): a ClassificationTask training step on the HIP path vs the CPU oracle
(oracle/torchok_ref.py) on identical seeded inputs and perturbed parameters.

bf16 end-to-end gradients of a deep BatchNorm/ReLU net differ from fp32 by far more than 1e-2 for
ANY bf16 implementation (ReLU masks / max-pool argmax flip under rounding): PyTorch's own
bf16-autocast CPU run of the oracle is used as the yardstick — the HIP path must be as close to the
fp32 oracle as torch-autocast is (x1.5 + 1e-2).  Tight (≤1e-2) checks are per-unit, teacher-forced,
in test_kernels_gpu.py / test_units_gpu.py."""
import copy

import pytest
import torch

import oracle.torchok_ref as R
import torchok_amd as T
from helpers import cls_config, copy_state, deterministic_state, perturb_, rel_err

pytestmark = pytest.mark.gpu


def _autocast_grads(ref, x, y):
    ref2 = copy.deepcopy(ref)
    with torch.autocast('cpu', dtype=torch.bfloat16):
        o = ref2.forward_with_gt({'image': x, 'target': y})
    loss = torch.nn.functional.cross_entropy(o['prediction'].float(), y)
    loss.backward()
    return float(loss), {n: p.grad for n, p in ref2.named_parameters()}


@pytest.mark.parametrize('backbone,size,batch,classes', [('resnet18', 64, 32, 10), ('resnet50', 96, 16, 1000)])
def test_training_step_vs_oracle(backbone, size, batch, classes):
    torch.manual_seed(0)
    cfg = cls_config(backbone, classes, backbone_params={'zero_init_last': False})
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
    ref = R.ClassificationModel(backbone, classes, zero_init_last=False)
    ref.load_state_dict(deterministic_state(ref.state_dict(), 21))
    copy_state(ref, task)
    task.cuda().train()
    ref.train()
    x = torch.randn(batch, 3, size, size)
    y = torch.randint(0, classes, (batch,))
    opt = task.configure_optimizers()[0]['optimizer']
    ropt = torch.optim.SGD(ref.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)

    ac_loss, ac_grads = _autocast_grads(ref, x, y)
    out = task.training_step({'image': x.cuda(), 'target': y.cuda()}, 0)
    assert set(out) == {'loss'}
    out['loss'].backward()
    ref_loss, ref_out = R.training_step(ref, {'image': x, 'target': y}, None)
    torch.cuda.synchronize()

    assert abs(float(out['loss']) - float(ref_loss)) < max(2e-2, 1.5 * abs(ac_loss - float(ref_loss)) + 1e-2)
    rp = dict(ref.named_parameters())
    for n, p in task.named_parameters():
        assert p.grad is not None, n
        mine = rel_err(p.grad, rp[n].grad)
        yard = rel_err(ac_grads[n], rp[n].grad)
        assert mine < 1.5 * yard + 1e-2, (n, mine, yard)
    # BatchNorm running statistics and the int64 step counter (exact)
    rb = dict(ref.named_buffers())
    for n, b in task.named_buffers():
        if n not in rb:
            continue
        if n.endswith('num_batches_tracked'):
            assert int(b) == int(rb[n]) == 1
        else:
            assert rel_err(b, rb[n]) < 5e-2, n   # bf16 conv outputs feed the batch variance
    # optimizer step on the arena == torch.optim.SGD given the same gradients
    with torch.no_grad():
        for n, p in ref.named_parameters():
            p.grad = dict(task.named_parameters())[n].grad.detach().cpu().float().contiguous().clone()
    before = {n: p.detach().cpu().clone() for n, p in task.named_parameters()}
    opt.step()
    ropt.step()
    torch.cuda.synchronize()
    for n, p in task.named_parameters():
        assert not torch.equal(p.detach().cpu(), before[n]) or p.grad.abs().sum() == 0
        assert rel_err(p, rp[n]) < 1e-5, n
    # second step runs (packs refreshed from the moved masters, momentum buffers initialised)
    opt.zero_grad()
    out2 = task.training_step({'image': x.cuda(), 'target': y.cuda()}, 1)
    out2['loss'].backward()
    opt.step()
    torch.cuda.synchronize()
    ref_loss2, _ = R.training_step(ref, {'image': x, 'target': y}, None)   # oracle after the same update
    assert torch.isfinite(out2['loss'])
    assert abs(float(out2['loss']) - float(ref_loss2)) < 0.15 * max(1.0, abs(float(ref_loss2)))


def test_forward_features_shapes():
    """reference tests/additional_tests/models/backbones/test_backbone.py:145-151 (resnet18 @ 2x3x64x64)."""
    m = T.BACKBONES.get('resnet18')(pretrained=False, in_channels=3).cuda().eval()
    x = torch.rand(2, 3, 64, 64, device='cuda')
    with torch.no_grad():
        last = m(x)
        feats = m.forward_features(x)
    assert tuple(last.shape) == (2, 512, 2, 2)
    assert [tuple(f.shape) for f in feats] == [(2, 3, 64, 64), (2, 64, 32, 32), (2, 64, 16, 16), (2, 128, 8, 8),
                                               (2, 256, 4, 4), (2, 512, 2, 2)]
    assert m.out_channels == 512 and m.out_encoder_channels == (64, 64, 128, 256, 512)


def test_eval_mode_uses_running_stats():
    torch.manual_seed(1)
    m = T.BACKBONES.get('resnet18')(pretrained=False).cuda()
    ref = R.resnet18()
    perturb_(ref, scale=0.1)
    with torch.no_grad():
        for b in ref.buffers():
            if b.dtype == torch.float32:
                b.add_(torch.rand_like(b) * 0.5)
    copy_state(ref, m)
    m.eval(), ref.eval()
    x = torch.randn(4, 3, 64, 64)
    with torch.no_grad():
        got = m(x.cuda()).float().cpu()
        want = ref(x)
    assert rel_err(got, want) < 3e-2


def test_cpu_tensor_is_rejected():
    m = T.BACKBONES.get('resnet18')(pretrained=False)
    with pytest.raises(RuntimeError, match='HIP'):
        m(torch.rand(1, 3, 32, 32))


def test_side_stream_schedule_is_bit_identical_and_learns(monkeypatch):
    """Race detector + end-to-end sanity: 40 SGD steps on a fixed mini-batch (a) drive the loss down, (b) give bit-identical
    parameters with the weight gradients on the side stream and on the main stream (every kernel is deterministic, so any
    cross-stream race would show up as a difference)."""
    from torchok_amd.engine import core as EC
    from torchok_amd.engine import functional as EF
    finals, losses = [], []
    for side in (True, False):
        monkeypatch.setattr(EF, 'WGRAD_SIDE_STREAM', side)
        monkeypatch.setattr(EC, 'BRANCH_STREAMS', side)
        cfg = cls_config('resnet18', 4, opt_params={'lr': 0.05, 'momentum': 0.9, 'weight_decay': 1e-4})
        task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
        sd = deterministic_state({k: v for k, v in task.state_dict().items() if not k.startswith('input_tensors')}, 5)
        task.load_state_dict(sd, strict=False)
        task.cuda().train()
        opt = task.configure_optimizers()[0]['optimizer']
        g = torch.Generator().manual_seed(7)
        x = torch.randn(32, 3, 64, 64, generator=g).cuda()
        y = torch.randint(0, 4, (32,), generator=g).cuda()
        hist = []
        for it in range(40):
            out = task.training_step({'image': x, 'target': y}, it)
            opt.zero_grad(set_to_none=True)
            out['loss'].backward()
            opt.step()
            hist.append(out['loss'].detach())
        torch.cuda.synchronize()
        losses.append([float(v) for v in hist])
        finals.append({n: p.detach().clone() for n, p in task.named_parameters()})
    assert losses[0][0] > 1.0 and losses[0][-1] < 0.2 * losses[0][0], (losses[0][0], losses[0][-1])
    assert losses[0] == losses[1]
    for n in finals[0]:
        assert torch.equal(finals[0][n], finals[1][n]), n


def test_hipgraph_replay_equals_eager():
    """GraphedTrainingStep (3 eager warm-up steps, one capture, n replays) leaves bit-identical parameters, BatchNorm buffers
    and loss to 3 + n eager steps: the captured graph holds exactly the kernels of one step."""
    from torchok_amd.engine.graph import GraphedTrainingStep
    n_replays = 4
    results = []
    for graphed in (False, True):
        cfg = cls_config('resnet18', 6, opt_params={'lr': 0.05, 'momentum': 0.9, 'weight_decay': 1e-4})
        task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
        sd = deterministic_state({k: v for k, v in task.state_dict().items() if not k.startswith('input_tensors')}, 9)
        task.load_state_dict(sd, strict=False)
        task.cuda().train()
        opt = task.configure_optimizers()[0]['optimizer']
        g = torch.Generator().manual_seed(11)
        batch = {'image': torch.randn(16, 3, 64, 64, generator=g).cuda(), 'target': torch.randint(0, 6, (16,), generator=g).cuda()}
        if graphed:
            step = GraphedTrainingStep(task, opt, batch, warmup=3)
            for _ in range(n_replays):
                loss = step(batch)['loss']
        else:
            for it in range(3 + n_replays):
                out = task.training_step(batch, it)
                opt.zero_grad(set_to_none=True)
                out['loss'].backward()
                opt.step()
                loss = out['loss']
        torch.cuda.synchronize()
        results.append((float(loss), {k: v.detach().clone() for k, v in task.state_dict().items()
                                      if not k.startswith('input_tensors')}))
    assert results[0][0] == results[1][0]
    for k in results[0][1]:
        assert torch.equal(results[0][1][k], results[1][1][k]), k


def test_fused_stem_pool_leaves_training_bit_identical(monkeypatch):
    """bn1 + ReLU + max-pool as one pass (engine.functional.FUSE_STEM_POOL; ResNet.forward only — forward_features still
    returns act1) against the unfused chain: 6 SGD steps, identical losses, parameters and BatchNorm buffers."""
    from torchok_amd.engine import functional as EF
    finals = []
    monkeypatch.setattr(EF, 'STEM_POOLED_STATS', False)      # position-domain sums: the bit-identical form
    for fuse in (True, False):
        monkeypatch.setattr(EF, 'FUSE_STEM_POOL', fuse)
        cfg = cls_config('resnet18', 6, opt_params={'lr': 0.05, 'momentum': 0.9, 'weight_decay': 1e-4})
        task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
        sd = deterministic_state({k: v for k, v in task.state_dict().items() if not k.startswith('input_tensors')}, 3)
        task.load_state_dict(sd, strict=False)
        task.cuda().train()
        opt = task.configure_optimizers()[0]['optimizer']
        g = torch.Generator().manual_seed(11)
        x, y = torch.randn(16, 3, 64, 64, generator=g).cuda(), torch.randint(0, 6, (16,), generator=g).cuda()
        losses = []
        for it in range(6):
            out = task.training_step({'image': x, 'target': y}, it)
            opt.zero_grad(set_to_none=True)
            out['loss'].backward()
            opt.step()
            losses.append(float(out['loss'].detach()))
        torch.cuda.synchronize()
        state = {n: v.detach().clone() for n, v in task.state_dict().items() if not n.startswith('input_tensors')}
        finals.append((losses, state))
        feats = task.backbone.forward_features(x)
        assert tuple(feats[1].shape) == (16, 64, 32, 32)                 # act1 is still there when asked for
    assert finals[0][0] == finals[1][0]
    for n in finals[0][1]:
        assert torch.equal(finals[0][1][n], finals[1][1][n]), n


def test_pooled_domain_stem_statistics_match_the_position_domain(monkeypatch):
    """engine.functional.STEM_POOLED_STATS (default): the BatchNorm-backward sums of the fused stem taken over the pooled
    elements.  One backward pass from the same state: every gradient above the stem is bit-identical, conv1 / bn1 agree
    to the bf16 rounding the position-domain form applies where several windows hit one position."""
    from torchok_amd.engine import functional as EF
    grads = []
    for pooled in (True, False):
        monkeypatch.setattr(EF, 'STEM_POOLED_STATS', pooled)
        cfg = cls_config('resnet18', 6)
        task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
        sd = deterministic_state({k: v for k, v in task.state_dict().items() if not k.startswith('input_tensors')}, 3)
        task.load_state_dict(sd, strict=False)
        task.cuda().train()
        g = torch.Generator().manual_seed(11)
        x, y = torch.randn(32, 3, 96, 96, generator=g).cuda(), torch.randint(0, 6, (32,), generator=g).cuda()
        task.training_step({'image': x, 'target': y}, 0)['loss'].backward()
        torch.cuda.synchronize()
        grads.append({n: p.grad.detach().float().clone() for n, p in task.named_parameters()})
    for n in grads[0]:
        if n.startswith('backbone.conv1') or n.startswith('backbone.bn1'):
            assert rel_err(grads[0][n], grads[1][n]) < 1e-2, n
        else:
            assert torch.equal(grads[0][n], grads[1][n]), n
