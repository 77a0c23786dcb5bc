"""BEiT on the MI355X: a teacher-forced Block and ClassificationTask steps against the restatement (tests/beit_ref.py) within the
bf16-autocast yardstick of test_vit_gpu.py (1.5 x the autocast distance + 1e-2), beit_base_patch16_224 for finiteness and
bit-identical reruns, the eval forward and the recipe through the fit loop."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

import beit_ref as R
import torchok_amd as T
from helpers import copy_state, rel_err
from torchok_amd import engine
from torchok_amd.models.backbones import beit as beit_mod

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
RECIPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'recipes')


@pytest.mark.parametrize('grid', [(2, 2), (8, 8)], ids=['5tok', '65tok'])
def test_teacher_forced_block_vs_restatement(grid):
    from functools import partial
    dim, heads, b = 128, 2, 3
    n = grid[0] * grid[1] + 1
    norm = partial(torch.nn.LayerNorm, eps=1e-6)
    ref = R.ref_state(R.Block(dim, heads, 4., True, norm, 0.1, grid), 7)
    blk = beit_mod.Block(dim, heads, 4., qkv_bias=True, init_values=0.1, norm_layer=norm, window_size=grid)
    copy_state(ref, blk)
    blk.cuda().train()
    g = torch.Generator().manual_seed(n)
    x = torch.randn(b, n, dim, generator=g).to(BF).float()            # the same bf16-representable input on both sides
    w = torch.randn(b, n, dim, generator=g).to(BF).float()            # the upstream gradient
    xr = x.clone().requires_grad_(True)
    (ref(xr) * w).sum().backward()
    ref2, xa = copy.deepcopy(ref), x.clone().requires_grad_(True)
    ref2.zero_grad()
    with torch.autocast('cpu', dtype=BF):
        oa = ref2(xa)
    (oa.float() * w).sum().backward()
    xd = x.reshape(b * n, dim).to(BF).cuda().requires_grad_(True)
    with engine.region() as r:
        out = r.output(blk.run(r, r.input(xd), b, n))
    out.backward(w.reshape(b * n, dim).to(BF).cuda())
    torch.cuda.synchronize()
    want = ref(x).detach()
    assert rel_err(out.float().cpu().view(b, n, dim), want) < 1.5 * rel_err(oa.float(), want) + 1e-2
    pairs = [('x', xd.grad.float().cpu().view(b, n, dim), xr.grad, xa.grad)]
    rp, ap = dict(ref.named_parameters()), dict(ref2.named_parameters())
    for name, p in blk.named_parameters():
        assert p.grad is not None, name
        pairs.append((name, p.grad, rp[name].grad, ap[name].grad))
    assert {nm for nm, *_ in pairs} >= {'gamma_1', 'gamma_2', 'attn.relative_position_bias_table', 'attn.q_bias', 'attn.v_bias'}
    for name, mine, fp32, ac in pairs:
        e, yard = rel_err(mine, fp32), rel_err(ac, fp32)
        print(f'block n={n} {name}: mine {e:.4g} autocast {yard:.4g}')
        assert e < 1.5 * yard + 1e-2, (name, e, yard)


def _task_and_ref(bp, optimizer='SGD', seed=3, classes=10):
    opt = {'SGD': None, 'AdamW': {'lr': 1e-3, 'weight_decay': 0.05}}[optimizer]
    task = R.beit_task(backbone_params=dict(R.TINY_BP, **bp), optimizer=optimizer, opt_params=opt, num_classes=classes)
    ref = R.ref_state(R.Classifier(classes, **R.TINY), seed)
    R.copy_backbone_state(ref, task)
    return task, ref


@pytest.mark.parametrize('drop_path', [0.0, 0.1])
def test_training_step_vs_restatement(drop_path):
    torch.manual_seed(0)
    task, ref = _task_and_ref(dict(drop_path_rate=drop_path), 'AdamW')
    task.cuda().train()
    ref.train()
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(8, 3, 64, 64, generator=g), torch.randint(0, 10, (8,), generator=g)
    orig = beit_mod.draw_drop_scales
    if drop_path:
        s1 = torch.tensor([1 / 0.9, 0.0, 1 / 0.9, 1 / 0.9, 0.0, 1 / 0.9, 1 / 0.9, 1 / 0.9])
        s2 = torch.tensor([0.0, 1 / 0.9, 1 / 0.9, 0.0, 1 / 0.9, 1 / 0.9, 1 / 0.9, 1 / 0.9])
        blk = task.backbone.blocks[1]
        assert type(task.backbone.blocks[0].drop_path1).__name__ == 'Identity'
        blk.drop_path1._drawn, blk.drop_path2._drawn = s1.cuda(), s2.cuda()
        ref.backbone.blocks[1].drop_scales = (s1, s2)
        beit_mod.draw_drop_scales = lambda *a, **k: None            # keep the pinned vectors
    ref2 = copy.deepcopy(ref)
    with torch.autocast('cpu', dtype=BF):
        ac_loss = F.cross_entropy(ref2(x).float(), y)
    ac_loss.backward()
    opt = task.configure_optimizers()[0]['optimizer']
    try:
        out = task.training_step({'image': x.cuda(), 'target': y.cuda()}, 0)
        out['loss'].backward()
    finally:
        beit_mod.draw_drop_scales = orig
    ref_loss = F.cross_entropy(ref(x), y)
    ref_loss.backward()
    torch.cuda.synchronize()
    assert abs(float(out['loss']) - float(ref_loss)) < max(2e-2, 1.5 * abs(float(ac_loss) - float(ref_loss)) + 1e-2)
    rp, ap = dict(ref.named_parameters()), dict(ref2.named_parameters())
    seen = set()
    for n, p in task.named_parameters():
        if n.startswith('backbone.fpn'):
            assert p.grad is None, n
            continue
        assert p.grad is not None, n
        mine, yard = rel_err(p.grad, rp[n].grad), rel_err(ap[n].grad, rp[n].grad)
        print(f'step dp={drop_path} {n}: mine {mine:.4g} autocast {yard:.4g}')
        assert mine < 1.5 * yard + 1e-2, (n, mine, yard)
        seen.add(n)
    assert seen == set(rp)
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in task.parameters())


def test_eval_forward_vs_restatement():
    task, ref = _task_and_ref({}, seed=4)
    task.cuda().eval()
    ref.eval()
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        mine = task.backbone(x.cuda()).float().cpu()
        want = ref.backbone(x)
        with torch.autocast('cpu', dtype=BF):
            ac = ref.backbone(x).float()
    assert tuple(mine.shape) == (4, 128, 1, 1)
    assert rel_err(mine, want) < 1.5 * rel_err(ac, want) + 1e-2


def test_abs_pos_emb_and_plain_residual_vs_restatement():
    """use_abs_pos_emb=True (pos_embed takes a gradient) and init_values=None (plain residual, no gammas)"""
    bp = dict(use_abs_pos_emb=True, init_values=None)
    task = R.beit_task(backbone_params=dict(R.TINY_BP, **bp))
    ref = R.ref_state(R.Classifier(10, **dict(R.TINY, **bp)), 6)
    R.copy_backbone_state(ref, task)
    task.cuda().train()
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(4, 3, 64, 64, generator=g), torch.randint(0, 10, (4,), generator=g)
    out = task.training_step({'image': x.cuda(), 'target': y.cuda()}, 0)
    out['loss'].backward()
    ref2 = copy.deepcopy(ref)
    with torch.autocast('cpu', dtype=BF):
        F.cross_entropy(ref2(x).float(), y).backward()
    F.cross_entropy(ref(x), y).backward()
    rp, ap = dict(ref.named_parameters()), dict(ref2.named_parameters())
    assert 'backbone.pos_embed' in rp and not any('gamma' in n for n in rp)
    for n, p in task.named_parameters():
        if n.startswith('backbone.fpn'):
            continue
        mine, yard = rel_err(p.grad, rp[n].grad), rel_err(ap[n].grad, rp[n].grad)
        assert mine < 1.5 * yard + 1e-2, (n, mine, yard)


def test_beit_base_b2_finite_and_bit_identical():
    g = torch.Generator().manual_seed(11)
    x, y = torch.randn(2, 3, 224, 224, generator=g).cuda(), torch.randint(0, 10, (2,), generator=g).cuda()
    runs = []
    for _ in range(2):
        torch.manual_seed(21)
        task = R.beit_task(side=224)
        with torch.no_grad():
            for n, p in task.named_parameters():
                if 'relative_position_bias_table' in n:
                    p.normal_(std=0.5)
        task.cuda().train()
        out = task.training_step({'image': x, 'target': y}, 0)
        out['loss'].backward()
        torch.cuda.synchronize()
        grads = {}
        for n, p in task.named_parameters():
            if n.startswith('backbone.fpn'):
                assert p.grad is None, n
            else:
                assert p.grad is not None and torch.isfinite(p.grad).all(), n
                grads[n] = p.grad.detach().clone()
        assert float(grads['backbone.blocks.0.attn.relative_position_bias_table'].abs().sum()) > 0
        runs.append((float(out['loss']), grads))
        del task
    assert runs[0][0] == runs[1][0]
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


def test_beit_recipe_through_the_fit_loop():
    from torchok_amd.run import fit
    os.environ.setdefault('HOME', '/root')
    cfg = T.load_config(os.path.join(RECIPES, 'classification_beit.yaml'), overrides={'trainer.devices': 1})
    assert cfg.task.params.backbone_name == 'beit_base_patch16_224'
    torch.manual_seed(0)
    seen = []
    batches = [{'image': torch.randn(4, 3, 64, 64).cuda(), 'target': torch.randint(0, 10, (4,)).cuda()} for _ in range(2)]
    res = fit(cfg, batches=batches, max_steps=2, device='cuda:0', on_step=lambda i, out: seen.append(float(out['loss'])))
    assert res['steps'] == 2 and len(seen) == 2 and all(v == v for v in seen)
