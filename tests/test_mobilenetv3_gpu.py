"""MobileNetV3 on the MI355X: teacher-forced blocks against the fp32 restatement (tests/mobilenetv3_ref.py),
ClassificationTask training steps against the oracle with the bf16-autocast yardstick of test_resnet_gpu.py, eval forward,
reproducibility, hipGraph replay and the recipe through the fit loop.  The kernels' own contracts are in
tests/test_hswish_contract_gpu.py."""
import copy
import os

import pytest
import torch

import mobilenetv3_ref as M
import oracle.torchok_ref as R
import torchok_amd as T
from helpers import cls_config, copy_state, deterministic_state, record_distance, rel_err
from torchok_amd import engine

pytestmark = pytest.mark.gpu
RECIPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'recipes')


def _gate(name):
    """x1.5 the bf16-autocast distance + 1e-2 (test_resnet_gpu.py).  The squeeze-excite conv_reduce gradients are the residual
    of a cancelling sum over each image of d(out) * x times the gate's derivative, formed from gradients stored in bf16, where
    autocast keeps that path in fp32: test_mnasnet_gpu.py::_gate gives them x6.0 with the sigmoid gate.  With the hard-sigmoid
    gate (derivative 1/6 or 0) the ratio of this build's distance to autocast's, measured on the device over every
    se.conv_reduce parameter of the block and training-step cases below, is at most 1.32 (blocks.2.1 of mobilenetv3_small_100 at
    64 x 64; profiles/mobilenetv3_gpu_tests.txt).  The factor is that ratio x 1.5 = 2.0, not the looser 6.0."""
    return 2.0 if 'se.conv_reduce.' in name else 1.5


def _block_pair(ref_block, eng_block, x, dout, what):
    """teacher-forced: the same bf16 input and output gradient into the oracle block (fp32 and bf16 autocast) and the engine
    block; output within 1e-2, every gradient within the autocast yardstick, running statistics within 1e-2."""
    eng_block.load_state_dict(ref_block.state_dict())
    eng_block.cuda().train()
    ref_block.train()
    ac_block = copy.deepcopy(ref_block)
    xa = x.float().requires_grad_()
    with torch.autocast('cpu', dtype=torch.bfloat16):
        ya = ac_block(xa)
    ya.float().backward(dout.float())
    xr = x.float().requires_grad_()
    yr = ref_block(xr)
    yr.backward(dout.float())
    xe = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    with engine.region() as r:
        t = r.input(xe)
        ye = r.output(eng_block(t))
    ye.backward(dout.cuda().contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    assert rel_err(ye, yr) <= 1e-2
    assert rel_err(xe.grad, xr.grad) < 1.5 * rel_err(xa.grad, xr.grad) + 1e-2
    rp, ap = dict(ref_block.named_parameters()), dict(ac_block.named_parameters())
    for name, prm in eng_block.named_parameters():
        mine, yard = rel_err(prm.grad, rp[name].grad), rel_err(ap[name].grad, rp[name].grad)
        record_distance(f'test_mobilenetv3_gpu::{what}', name, hip_vs_fp32=mine, autocast_vs_fp32=yard)
        assert mine < _gate(name) * yard + 1e-2, (name, mine, yard)
    rb = dict(ref_block.named_buffers())
    for name, b in eng_block.named_buffers():
        if b.is_floating_point():
            assert rel_err(b, rb[name]) <= 1e-2, name


def _perturbed(block):
    with torch.no_grad():
        for name, prm in block.named_parameters():
            if prm.dim() == 1:
                prm.add_(torch.randn_like(prm) * 0.2 + (0.5 if name.endswith('bn3.weight') else 0.0))
    return block


BLOCKS = {  # name -> (class, arguments, input channels, output channels, stride)
    'ds_se_relu_s2': ('DepthwiseSeparableConv', (16, 16, 3, 2, False, 0.25, True), 16, 16, 2),
    'ir_hswish_se_k5_skip': ('InvertedResidual', (40, 40, 5, 1, False, 6.0, 0.25, False), 40, 40, 1),
    'ir_hswish_k3_s2': ('InvertedResidual', (40, 80, 3, 2, False, 6.0, 0.0, False), 40, 80, 2),
    'cn_hswish': ('ConvBnAct', (96, 576, 1, 1, False), 96, 576, 1),
}


@pytest.mark.parametrize('what', sorted(BLOCKS))
def test_block_vs_oracle(what):
    from torchok_amd.models.backbones import mobilenetv3 as V3
    cls, args, cin, cout, s = BLOCKS[what]
    torch.manual_seed(0)
    ref = _perturbed(getattr(M, cls)(*args))
    eng = getattr(V3, cls)(*args)
    assert eng.has_skip == (what == 'ir_hswish_se_k5_skip')
    g = torch.Generator().manual_seed(1)
    x = torch.randn(8, cin, 28, 28, generator=g).to(torch.bfloat16)
    ho = (28 - 1) // s + 1
    dout = torch.randn(8, cout, ho, ho, generator=g).to(torch.bfloat16)
    _block_pair(ref, eng, x, dout, what)


def _task_and_ref(name, classes=10, seed=21):
    cfg = cls_config(name, classes)
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
    ref = M.Classifier(name, classes)
    ref.load_state_dict(deterministic_state(ref.state_dict(), seed))
    copy_state(ref, task)
    return task, ref


def _step_vs_oracle(name, x, y):
    torch.manual_seed(0)
    task, ref = _task_and_ref(name)
    task.cuda().train()
    ref.train()
    ref2 = copy.deepcopy(ref)
    with torch.autocast('cpu', dtype=torch.bfloat16):
        o = ref2.forward_with_gt({'image': x, 'target': y})
    ac_loss = torch.nn.functional.cross_entropy(o['prediction'].float(), y)
    ac_loss.backward()
    ac_grads = {n: p.grad for n, p in ref2.named_parameters()}
    out = task.training_step({'image': x.cuda(), 'target': y.cuda()}, 0)
    out['loss'].backward()
    ref_loss, _ = R.training_step(ref, {'image': x, 'target': y}, None)
    torch.cuda.synchronize()
    assert abs(float(out['loss']) - float(ref_loss)) < max(2e-2, 1.5 * abs(float(ac_loss) - float(ref_loss)) + 1e-2)
    rp = dict(ref.named_parameters())
    for n, p in task.named_parameters():
        assert p.grad is not None, n
        scale = M.grad_scale(n, rp)          # (the analytically zero gradients: see its docstring)
        mine, yard = M.dist(p.grad, rp[n].grad, scale), M.dist(ac_grads[n], rp[n].grad, scale)
        record_distance(f'test_mobilenetv3_gpu::step[{name},{x.shape[2]}x{x.shape[3]}]', n, hip_vs_fp32=mine, autocast_vs_fp32=yard)
        assert mine < _gate(n) * yard + 1e-2, (n, mine, yard)


@pytest.mark.parametrize('name', ['mobilenetv3_small_100', 'mobilenetv3_large_100'])
def test_training_step_vs_oracle(name):
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(8, 3, 64, 64, generator=g), torch.randint(0, 10, (8,), generator=g)
    _step_vs_oracle(name, x, y)


def test_training_step_non_square_vs_oracle():
    """sides that are not multiples of 32: every depthwise and squeeze-excite layer sees a non-square map"""
    g = torch.Generator().manual_seed(6)
    x, y = torch.randn(8, 3, 100, 140, generator=g), torch.randint(0, 10, (8,), generator=g)
    _step_vs_oracle('mobilenetv3_small_100', x, y)


def test_eval_forward_vs_oracle():
    task, ref = _task_and_ref('mobilenetv3_large_100', seed=4)
    task.cuda().eval()
    ref.eval()
    x = torch.randn(8, 3, 96, 96, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        mine = task.backbone(x.cuda()).float().cpu()
        want = ref.backbone(x)
        with torch.autocast('cpu', dtype=torch.bfloat16):
            ac = ref.backbone(x).float()
        feats = task.backbone.forward_features(x.cuda())
        want_feats = ref.backbone.forward_features(x)
    assert rel_err(mine, want) < 1.5 * rel_err(ac, want) + 1e-2
    assert [tuple(f.shape) for f in feats] == [tuple(f.shape) for f in want_feats]
    for a, b in zip(feats[1:], want_feats[1:]):
        assert rel_err(a.float().cpu(), b) < 5e-2


def _steps(task, opt, batch, n):
    losses = []
    for it in range(n):
        out = task.training_step(batch, it)
        opt.zero_grad(set_to_none=True)
        out['loss'].backward()
        opt.step()
        losses.append(float(out['loss']))
    torch.cuda.synchronize()
    return losses


def _batch(classes=6):
    g = torch.Generator().manual_seed(11)
    return {'image': torch.randn(16, 3, 64, 64, generator=g).cuda(), 'target': torch.randint(0, classes, (16,), generator=g).cuda()}


def _state(task):
    return {k: v.detach().clone() for k, v in task.state_dict().items() if not k.startswith('input_tensors')}


def test_two_runs_are_bit_identical():
    results = []
    batch = _batch()
    for _ in range(2):
        task, _ = _task_and_ref('mobilenetv3_small_100', 6, seed=9)
        task.cuda().train()
        losses = _steps(task, task.configure_optimizers()[0]['optimizer'], batch, 2)
        results.append((losses, _state(task)))
    assert results[0][0] == results[1][0]
    for k in results[0][1]:
        assert torch.equal(results[0][1][k], results[1][1][k]), k


def test_hipgraph_replay_equals_eager():
    from torchok_amd.engine.graph import GraphedTrainingStep
    batch = _batch()
    results = []
    for graphed in (False, True):
        task, _ = _task_and_ref('mobilenetv3_small_100', 6, seed=9)
        task.cuda().train()
        opt = task.configure_optimizers()[0]['optimizer']
        if graphed:
            step = GraphedTrainingStep(task, opt, batch, warmup=3)
            for _ in range(2):
                loss = float(step(batch)['loss'])
        else:
            loss = _steps(task, opt, batch, 5)[-1]
        torch.cuda.synchronize()
        results.append((loss, _state(task)))
    assert results[0][0] == results[1][0]
    for k in results[0][1]:
        assert torch.equal(results[0][1][k], results[1][1][k]), k


def test_recipe_fit_on_device():
    from torchok_amd.run import fit
    cfg = T.load_config(os.path.join(RECIPES, 'classification_mobilenetv3.yaml'), overrides={'trainer.devices': 1})
    assert cfg.task.params.backbone_name == 'mobilenetv3_small_100'
    g = torch.Generator().manual_seed(0)
    batches = [{'image': torch.randn(8, 3, 64, 64, generator=g).cuda(), 'target': torch.randint(0, 10, (8,), generator=g).cuda()}
               for _ in range(2)]
    seen = []
    res = fit(cfg, batches=batches, max_steps=2, device='cuda:0', on_step=lambda i, out: seen.append(float(out['loss'])))
    assert res['steps'] == 2 and len(seen) == 2 and all(v == v and abs(v) != float('inf') for v in seen)
