"""GCViT on the MI355X against the plain-torch restatement (tests/gcvit_ref.py): a small model teacher-forced (output, every
parameter gradient, the input gradient of a stage), ClassificationTask training steps of gcvit_xxtiny and gcvit_small, eval
forward, reproducibility and the recipe through the fit loop.  The gate is the project's own (test_resnet_gpu.py): as close to
the fp32 CPU run as torch's bf16-autocast CPU run, x1.5 + 1e-2 on rel_err; for a scalar loss max(2e-2, 1.5 autocast + 1e-2).
The kernels' own contracts are in tests/test_gc_attn_contract_gpu.py."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

import gcvit_ref as R
import torchok_amd as T
from helpers import cls_config, copy_state, record_distance, rel_err

pytestmark = pytest.mark.gpu
RECIPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'recipes')
BF = torch.bfloat16


def _gated(tag, name, mine, yard):
    record_distance(f'test_gcvit_gpu::{tag}', name, hip_vs_fp32=mine, autocast_vs_fp32=yard)
    print(f'{tag} {name} hip {mine:.4f} autocast {yard:.4f}')
    return mine < 1.5 * yard + 1e-2


def test_small_model_teacher_forced():
    """GlobalContextVit(img_size=224, embed_dim=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8)): windows 7 / 7 / 14 / 7, a
    local and a global block in every stage; the same image and output gradient into the restatement (fp32 and bf16 autocast)
    and the engine"""
    from torchok_amd.models.backbones.gcvit import GlobalContextVit
    torch.manual_seed(0)
    ref = R.ref_state(R.GlobalContextVit(**R.SMALL), 7).train()
    m = GlobalContextVit(**R.SMALL)
    m.load_state_dict(ref.state_dict())
    m.cuda().train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 224, 224, generator=g)
    dout = torch.randn(2, 256, 7, 7, generator=g).to(BF)
    ac = copy.deepcopy(ref)
    with torch.autocast('cpu', dtype=BF):
        ya = ac(x)
    ya.float().backward(dout.float())
    yr = ref(x)
    yr.backward(dout.float())
    ye = m(x.cuda())
    ye.backward(dout.cuda())
    torch.cuda.synchronize()
    assert tuple(ye.shape) == (2, 256, 7, 7)
    bad = []
    if not _gated('small', 'output', rel_err(ye, yr), rel_err(ya, yr)):
        bad.append('output')
    rp, ap = dict(ref.named_parameters()), dict(ac.named_parameters())
    assert {n for n, _ in m.named_parameters()} == set(rp)
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        if not _gated('small', n, rel_err(p.grad, rp[n].grad), rel_err(ap[n].grad, rp[n].grad)):
            bad.append(n)
    assert not bad, bad


def test_stage_input_gradient_teacher_forced():
    """the image takes no gradient in this engine; the input of a stage does.  Stage 1 of the small model at B = 2: its input
    feeds the downsample only, the downsampled map feeds the first block and the global_block (28 x 28, windows of 7, nW = 16)"""
    from torchok_amd.models.backbones.gcvit import GlobalContextVit
    torch.manual_seed(0)
    ref = R.ref_state(R.GlobalContextVit(**R.SMALL), 8).stages[1].train()
    m = GlobalContextVit(**R.SMALL).stages[1]
    m.load_state_dict(ref.state_dict())
    m.cuda().train()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 32, 56, 56, generator=g).to(BF)
    dout = torch.randn(2, 64, 28, 28, generator=g).to(BF)
    ac = copy.deepcopy(ref)
    xa = x.float().requires_grad_()
    with torch.autocast('cpu', dtype=BF):
        ya = ac(xa)
    ya.float().backward(dout.float())
    xr = x.float().requires_grad_()
    yr = ref(xr)
    yr.backward(dout.float())
    xe = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    ye = m(xe)
    ye.backward(dout.cuda().contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    assert _gated('stage1', 'output', rel_err(ye, yr), rel_err(ya, yr))
    assert _gated('stage1', 'd(input)', rel_err(xe.grad, xr.grad), rel_err(xa.grad, xr.grad))


def _task_and_ref(name, seed):
    cfg = cls_config(name, 10, optimizer='AdamW', opt_params={'lr': 5e-4, 'weight_decay': 0.05}, inputs_shape=(3, 224, 224))
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
    ref = R.ref_state(R.Classifier(10, **R.VARIANTS[name]), seed)
    copy_state(ref, task)
    return task, ref


@pytest.mark.parametrize('name', ['gcvit_xxtiny', 'gcvit_small'])
def test_training_step_vs_restatement(name):
    """one AdamW step at B = 2, 224 x 224; gcvit_small runs the LayerScale residuals and the E = 96 widths (24-wide SE)"""
    torch.manual_seed(0)
    task, ref = _task_and_ref(name, seed=11)
    task.cuda().train()
    ref.train()
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(2, 3, 224, 224, generator=g), torch.randint(0, 10, (2,), generator=g)
    ac = copy.deepcopy(ref)
    with torch.autocast('cpu', dtype=BF):
        o = ac(x)
    ac_loss = F.cross_entropy(o.float(), y)
    ac_loss.backward()
    ref_loss = F.cross_entropy(ref(x), y)
    ref_loss.backward()
    opt = task.configure_optimizers()[0]['optimizer']
    out = task.training_step({'image': x.cuda(), 'target': y.cuda()}, 0)
    out['loss'].backward()
    torch.cuda.synchronize()
    print(name, 'loss', float(out['loss'].detach()), float(ref_loss.detach()), float(ac_loss.detach()))
    assert abs(float(out['loss']) - float(ref_loss)) < max(2e-2, 1.5 * abs(float(ac_loss) - float(ref_loss)) + 1e-2)
    rp, ap = dict(ref.named_parameters()), dict(ac.named_parameters())
    bad = []
    for n, p in task.named_parameters():
        assert p.grad is not None, n
        if not _gated(f'step[{name}]', n, rel_err(p.grad, rp[n].grad), rel_err(ap[n].grad, rp[n].grad)):
            bad.append(n)
    assert not bad, bad
    before = task.backbone.stem.conv1.weight.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(before, task.backbone.stem.conv1.weight.detach())
    assert all(torch.isfinite(p).all() for p in task.parameters())


def test_eval_forward_vs_restatement():
    task, ref = _task_and_ref('gcvit_xxtiny', seed=4)
    task.cuda().eval()
    ref.eval()
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        mine = task.backbone(x.cuda()).float().cpu()
        want = ref.backbone(x)
        with torch.autocast('cpu', dtype=BF):
            ac = ref.backbone(x).float()
        feats = task.backbone.forward_features(x.cuda())
        want_feats = ref.backbone.forward_features(x)
    assert _gated('eval', 'output', rel_err(mine, want), rel_err(ac, want))
    assert [tuple(f.shape) for f in feats] == [tuple(f.shape) for f in want_feats]
    for a, b in zip(feats[1:], want_feats[1:]):
        assert rel_err(a.float().cpu(), b) < 5e-2


def test_two_identical_steps_give_bit_identical_gradients():
    g = torch.Generator().manual_seed(11)
    batch = {'image': torch.randn(3, 3, 224, 224, generator=g).cuda(), 'target': torch.randint(0, 10, (3,), generator=g).cuda()}
    grads = []
    for _ in range(2):
        task, _ = _task_and_ref('gcvit_xxtiny', seed=9)
        task.cuda().train()
        out = task.training_step(batch, 0)
        out['loss'].backward()
        torch.cuda.synchronize()
        grads.append((float(out['loss']), {n: p.grad.detach().clone() for n, p in task.named_parameters()}))
    assert grads[0][0] == grads[1][0]
    for n in grads[0][1]:
        assert torch.equal(grads[0][1][n], grads[1][1][n]), n


@pytest.mark.parametrize('name', ['gcvit_xxtiny', 'gcvit_tiny'])
def test_recipe_fit_on_device(name):
    from torchok_amd.run import fit
    os.environ.setdefault('HOME', '/root')
    cfg = T.load_config(os.path.join(RECIPES, 'classification_gcvit_xxtiny.yaml'),
                        overrides={'trainer.devices': 1, 'task.params.backbone_name': name})
    assert cfg.task.params.backbone_name == name
    g = torch.Generator().manual_seed(0)
    batches = [{'image': torch.randn(2, 3, 224, 224, generator=g).cuda(), 'target': torch.randint(0, 10, (2,), generator=g).cuda()}
               for _ in range(2)]
    seen = []
    res = fit(cfg, batches=batches, max_steps=2, device='cuda:0', on_step=lambda i, out: seen.append(float(out['loss'])))
    assert res['steps'] == 2 and len(seen) == 2 and all(v == v and abs(v) != float('inf') for v in seen)
