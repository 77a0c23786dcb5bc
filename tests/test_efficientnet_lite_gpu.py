"""EfficientNet-Lite on the MI355X: teacher-forced blocks against the fp32 restatement (tests/efficientnet_lite_ref.py), a
ClassificationTask training step against the oracle with the bf16-autocast yardstick of test_mnasnet_gpu.py, the eval
forward, reproducibility and the recipe through the fit loop.  The kernels' own contracts are in
tests/test_relu6_contract_gpu.py."""
import copy
import os

import pytest
import torch

import efficientnet_lite_ref as L
import oracle.torchok_ref as R
import torchok_amd as T
from helpers import cls_config, copy_state, deterministic_state, record_distance, rel_err
from test_efficientnet_lite import BLOCKS, block_pair, perturbed

pytestmark = pytest.mark.gpu
RECIPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'recipes')
BF = torch.bfloat16


@pytest.mark.parametrize('what', sorted(BLOCKS))
def test_block_vs_oracle(what):
    make_ref, make_eng, cin, cout, s = BLOCKS[what]
    torch.manual_seed(0)
    ref, eng = perturbed(make_ref()), make_eng()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(8, cin, 14, 14, generator=g).to(BF)
    dout = torch.randn(8, cout, 14 // s, 14 // s, generator=g).to(BF)
    block_pair(ref, eng, x, dout, 'cuda', record=lambda name, mine, yard: record_distance(
        f'test_efficientnet_lite_gpu::{what}', name, hip_vs_fp32=mine, autocast_vs_fp32=yard))


def _task_and_ref(name, classes=10, seed=21):
    cfg = cls_config(name, classes)
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
    ref = L.Classifier(name, classes)
    ref.load_state_dict(deterministic_state(ref.state_dict(), seed))
    copy_state(ref, task)
    return task, ref


def _batch(n=2, classes=10, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, 64, 64, generator=g), torch.randint(0, classes, (n,), generator=g)


def test_training_step_vs_oracle():
    """efficientnet_lite0 at B = 2, 64 x 64 (the final map is 2 x 2: 8 samples per BatchNorm channel): the loss, every parameter
    gradient (x1.5 the bf16-autocast distance + 1e-2, test_mnasnet_gpu.py) and the running statistics."""
    name = 'efficientnet_lite0'
    x, y = _batch()
    torch.manual_seed(0)
    task, ref = _task_and_ref(name)
    task.cuda().train()
    ref.train()
    ref2 = copy.deepcopy(ref)
    with torch.autocast('cpu', dtype=BF):
        o = ref2.forward_with_gt({'image': x, 'target': y})
    ac_loss = torch.nn.functional.cross_entropy(o['prediction'].float(), y)
    ac_loss.backward()
    ac_grads = {n: p.grad for n, p in ref2.named_parameters()}
    out = task.training_step({'image': x.cuda(), 'target': y.cuda()}, 0)
    out['loss'].backward()
    ref_loss, _ = R.training_step(ref, {'image': x, 'target': y}, None)
    torch.cuda.synchronize()
    print(f'loss {float(out["loss"].detach()):.6f} fp32 {float(ref_loss):.6f} autocast {float(ac_loss.detach()):.6f}')
    assert abs(float(out['loss'].detach()) - float(ref_loss)) < max(2e-2, 1.5 * abs(float(ac_loss) - float(ref_loss)) + 1e-2)
    rp = dict(ref.named_parameters())
    assert {n for n, _ in task.named_parameters()} == set(rp)
    worst = (0.0, None)
    failures = []
    for n, p in task.named_parameters():
        assert p.grad is not None, n
        scale = L.grad_scale(n, rp)          # (the analytically zero gradients: see mobilenetv3_ref.grad_scale)
        mine, yard = L.dist(p.grad, rp[n].grad, scale), L.dist(ac_grads[n], rp[n].grad, scale)
        record_distance(f'test_efficientnet_lite_gpu::step[{name},64x64]', n, hip_vs_fp32=mine, autocast_vs_fp32=yard)
        worst = max(worst, (mine / (1.5 * yard + 1e-2), n))
        if not mine < 1.5 * yard + 1e-2:
            failures.append((n, mine, yard))
    print(f'worst gradient distance / bound: {worst[0]:.3f} ({worst[1]})')
    assert not failures, failures
    rb, ab = dict(ref.named_buffers()), dict(ref2.named_buffers())
    for n, b in task.named_buffers():
        if n in rb and b.is_floating_point():
            mine, yard = rel_err(b, rb[n]), rel_err(ab[n], rb[n])
            record_distance(f'test_efficientnet_lite_gpu::step[{name},64x64]', n, hip_vs_fp32=mine, autocast_vs_fp32=yard)
            assert mine < 1.5 * yard + 1e-2, (n, mine, yard)
        elif n in rb:
            assert int(b) == int(rb[n]) == 1, n


def test_eval_forward_vs_oracle():
    task, ref = _task_and_ref('efficientnet_lite0', seed=4)
    task.cuda().eval()
    ref.eval()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        mine = task.backbone(x.cuda()).float().cpu()
        want = ref.backbone(x)
        with torch.autocast('cpu', dtype=BF):
            ac = ref.backbone(x).float()
        feats = task.backbone.forward_features(x.cuda())
        want_feats = ref.backbone.forward_features(x)
    assert rel_err(mine, want) < 1.5 * rel_err(ac, want) + 1e-2
    assert [tuple(f.shape) for f in feats] == [tuple(f.shape) for f in want_feats]
    for a, b in zip(feats[1:], want_feats[1:]):
        assert rel_err(a.float().cpu(), b) < 5e-2


def test_lite4_constructs_and_runs_an_eval_forward():
    """the deepest and widest member (30 blocks, up to 1632 expanded channels): construction and one eval forward at 64 x 64"""
    task, ref = _task_and_ref('efficientnet_lite4', seed=4)
    assert [len(s) for s in task.backbone.blocks] == [1, 4, 4, 6, 6, 8, 1]
    assert max(m.num_features for m in task.backbone.modules() if isinstance(m, torch.nn.BatchNorm2d)) == 1632
    task.cuda().eval()
    ref.eval()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        mine = task.backbone(x.cuda()).float().cpu()
        want = ref.backbone(x)
        with torch.autocast('cpu', dtype=BF):
            ac = ref.backbone(x).float()
    assert tuple(mine.shape) == (2, 1280, 2, 2)
    assert rel_err(mine, want) < 1.5 * rel_err(ac, want) + 1e-2


def test_two_identical_steps_give_identical_gradients():
    x, y = _batch(seed=11)
    batch = {'image': x.cuda(), 'target': y.cuda()}
    grads = []
    for _ in range(2):
        torch.manual_seed(0)
        task, _ = _task_and_ref('efficientnet_lite0', seed=9)
        task.cuda().train()
        out = task.training_step(batch, 0)
        out['loss'].backward()
        torch.cuda.synchronize()
        grads.append((float(out['loss']), {n: p.grad.detach().clone() for n, p in task.named_parameters()},
                      {n: b.detach().clone() for n, b in task.named_buffers() if not n.startswith('input_tensors')}))
    assert grads[0][0] == grads[1][0]
    for part in (1, 2):
        for n in grads[0][part]:
            assert torch.equal(grads[0][part][n], grads[1][part][n]), n


def test_recipe_fit_on_device():
    from torchok_amd.run import fit
    cfg = T.load_config(os.path.join(RECIPES, 'classification_efficientnet_lite0.yaml'), overrides={'trainer.devices': 1})
    assert cfg.task.params.backbone_name == 'efficientnet_lite0'
    g = torch.Generator().manual_seed(0)
    batches = [{'image': torch.randn(2, 3, 64, 64, generator=g).cuda(), 'target': torch.randint(0, 10, (2,), generator=g).cuda()}
               for _ in range(2)]
    seen = []
    res = fit(cfg, batches=batches, max_steps=2, device='cuda:0', on_step=lambda i, out: seen.append(float(out['loss'])))
    assert res['steps'] == 2 and len(seen) == 2 and all(v == v and abs(v) != float('inf') for v in seen)
