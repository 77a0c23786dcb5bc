"""Gradient clipping kernels (csrc/grad_clip.hip) on the MI355X: torchok_amd.optim.clip_grad_norm_ / clip_grad_value_ against
torch.nn.utils and an fp64 reference, arena padding and stale slots left alone, and the clip inside train_step and a recorded
GraphedTrainingStep."""
import pytest
import torch

import torchok_amd as T
from helpers import cls_config, deterministic_state
from torchok_amd.engine.step import train_step
from torchok_amd.optim import clip_grad_norm_, clip_grad_value_

pytestmark = pytest.mark.gpu

ODD = [(1,), (3,), (63,), (65,)]


def _resnet50_shapes():
    cfg = cls_config('resnet50', 1000)
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
    shapes = [tuple(p.shape) for p in task.parameters()]
    assert len(shapes) == 161 and 25.5e6 < sum(torch.Size(s).numel() for s in shapes) < 25.6e6
    return shapes


@pytest.fixture(scope='module')
def shapes():
    return _resnet50_shapes() + ODD


def _setup(shapes, seed=0, stale=(5, 40, 161), scale=1e-3):
    """SGD over two groups (two arenas).  Every gradient byte of the arenas (padding, stale slots) is NaN first; the
    parameters listed in `stale` get no gradient, the others a random one written into their slot."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    params = [torch.nn.Parameter(torch.zeros(s, device='cuda')) for s in shapes]
    half = len(params) // 2
    opt = T.OPTIMIZERS.get('SGD')([{'params': params[:half]}, {'params': params[half:]}], lr=0.1)
    opt._ensure_built()
    for a in opt._arenas:
        a.grad.fill_(float('nan'))
    for i, p in enumerate(params):
        if i in stale:
            p.grad = None
            continue
        a = opt._arenas[0] if i < half else opt._arenas[1]
        j = i if i < half else i - half
        a.grad_view(j).copy_(torch.randn(p.shape, device='cuda', generator=g) * scale)
        p.grad = a.gviews[j]
    return params, opt


def _outside_bits(opt, params):
    """int32 bits of every arena word that is not the gradient of a parameter which has one (padding + stale slots)."""
    out = []
    for a in opt._arenas:
        mask = torch.ones(a.total, dtype=torch.bool, device='cuda')
        for i, p in enumerate(a.params):
            if p.grad is not None:
                mask[a.offsets[i]:a.offsets[i] + p.numel()] = False
        out.append(a.grad.view(torch.int32)[mask].clone())
    return out


def _grads(params):
    return [p.grad.detach().clone() for p in params if p.grad is not None]


def test_norm_and_scale_on_resnet50_shapes(shapes):
    params, opt = _setup(shapes)
    grads = _grads(params)
    outside = _outside_bits(opt, params)
    ref64 = float(torch.cat([g.double().flatten() for g in grads]).norm())
    ref_t = float(torch.nn.utils.get_total_norm(grads))
    # no clip: the norm, twice bit-identical, and the gradients untouched
    n1 = clip_grad_norm_(opt, 1e9)
    n2 = clip_grad_norm_(opt, 1e9)
    assert n1.dim() == 0 and n1.dtype == torch.float32 and n1.is_cuda
    assert torch.equal(n1.view(torch.int32), n2.view(torch.int32))
    assert abs(float(n1) - ref64) <= 2e-7 * ref64, (float(n1), ref64)
    assert abs(float(n1) - ref_t) <= 1e-5 * ref_t
    for a, b in zip(_grads(params), grads):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # clip: within 1e-6 of torch's
    max_norm = ref64 / 3
    coef = min(max_norm / (ref_t + 1e-6), 1.0)
    want = [g * torch.tensor(coef, dtype=torch.float32, device='cuda') for g in grads]
    n = clip_grad_norm_(opt, max_norm)
    assert abs(float(n) - ref64) <= 2e-7 * ref64
    for a, b in zip(_grads(params), want):
        assert (a - b).abs().max() <= 1e-6 * b.abs().max().clamp_min(1e-30)
    # padding and stale slots: neither read (the norm would be NaN) nor written
    for a, b in zip(_outside_bits(opt, params), outside):
        assert torch.equal(a, b)
    torch.cuda.synchronize()


def _torch_params(grads):
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    return ps


def test_clip_equals_torch_clip_grad_norm(shapes):
    params, opt = _setup(shapes, seed=1)
    ref = _torch_params(_grads(params))
    n_ref = torch.nn.utils.clip_grad_norm_(ref, 0.5)
    assert float(n_ref) > 0.5
    n = clip_grad_norm_(opt, 0.5)
    assert abs(float(n) - float(n_ref)) <= 1e-5 * float(n_ref)
    for a, b in zip(_grads(params), ref):
        assert (a - b.grad).abs().max() <= 1e-6 * b.grad.abs().max()


def test_non_finite_follows_torch(shapes):
    for bad in (float('nan'), float('inf')):
        params, opt = _setup(shapes, seed=2)
        params[7].grad.view(-1)[3] = bad
        ref = _torch_params(_grads(params))
        n_ref = torch.nn.utils.clip_grad_norm_(ref, 1.0)
        n = clip_grad_norm_(opt, 1.0)
        if bad != bad:
            assert torch.isnan(n) and torch.isnan(n_ref)
            assert all(torch.isnan(g).all() for g in _grads(params))
        else:
            assert float(n) == float('inf') and float(n_ref) == float('inf')
            assert float(opt._clip_state.scalars[1]) == 0.0
        for a, b in zip(_grads(params), ref):
            assert torch.equal(torch.isnan(a), torch.isnan(b.grad))
            assert torch.equal(a == 0, b.grad == 0)
        with pytest.raises(RuntimeError, match='non-finite'):
            clip_grad_norm_(opt, 1.0, error_if_nonfinite=True)


def test_clip_value_is_bit_identical_to_torch(shapes):
    params, opt = _setup(shapes, seed=3)
    params[2].grad.view(-1)[0] = float('nan')
    params[9].grad.view(-1)[1] = float('-inf')
    outside = _outside_bits(opt, params)
    ref = _torch_params(_grads(params))
    torch.nn.utils.clip_grad_value_(ref, 1e-3)
    clip_grad_value_(opt, 1e-3)
    for a, b in zip(_grads(params), ref):
        assert torch.equal(a.view(torch.int32), b.grad.view(torch.int32))
    assert torch.isnan(params[2].grad.view(-1)[0])
    for a, b in zip(_outside_bits(opt, params), outside):
        assert torch.equal(a, b)


def _resnet18_task(opt_name='SGD', opt_params=None):
    cfg = cls_config('resnet18', 6, optimizer=opt_name,
                     opt_params=opt_params or {'lr': 0.05, 'momentum': 0.9, 'weight_decay': 1e-4})
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
    sd = deterministic_state({k: v for k, v in task.state_dict().items() if not k.startswith('input_tensors')}, 9)
    task.load_state_dict(sd, strict=False)
    task.cuda().train()
    return task, task.configure_optimizers()[0]['optimizer']


def _batch():
    g = torch.Generator().manual_seed(11)
    return {'image': torch.randn(16, 3, 64, 64, generator=g).cuda(), 'target': torch.randint(0, 6, (16,), generator=g).cuda()}


def test_train_step_clip_equals_torch_clip_inserted_by_hand():
    max_norm = 0.5
    batch = _batch()
    task, opt = _resnet18_task()
    for i in range(3):
        train_step(task, opt, batch, i, clip=('norm', max_norm))
    ours = {k: v.detach().clone() for k, v in task.state_dict().items() if not k.startswith('input_tensors')}
    task, opt = _resnet18_task()
    norms = []
    for i in range(3):
        out = task.training_step(batch, i)
        opt.zero_grad(set_to_none=True)
        out['loss'].backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_([p for p in task.parameters() if p.grad is not None], max_norm)))
        opt.step()
        task.on_train_batch_end(out, batch, i)
    assert any(n > max_norm for n in norms), norms
    for k, v in task.state_dict().items():
        if k.startswith('input_tensors') or not v.is_floating_point():
            continue
        assert (ours[k] - v).norm() <= 1e-6 * v.norm().clamp_min(1e-12), k


@pytest.mark.parametrize('opt_name,opt_params', [('SGD', None),
                                                 ('AdamW', {'lr': 1e-5, 'weight_decay': 0.05, 'capturable': True})])
def test_graphed_step_with_clip_equals_eager(opt_name, opt_params):
    """The clip recorded with the step: replay equals eager bit for bit (and the recording has no host sync in it)."""
    from torchok_amd.engine.graph import GraphedTrainingStep
    n_replays, clip = 4, ('norm', 0.05)
    results = []
    for graphed in (False, True):
        task, opt = _resnet18_task(opt_name, opt_params)
        batch = _batch()
        coefs = []
        if graphed:
            step = GraphedTrainingStep(task, opt, batch, warmup=3, clip=clip)
            for _ in range(n_replays):
                loss = step(batch)['loss']
                coefs.append(float(opt._clip_state.scalars[1]))
        else:
            for it in range(3 + n_replays):
                loss = train_step(task, opt, batch, it, clip=clip, batch_end_hook=False)['loss']
                coefs.append(float(opt._clip_state.scalars[1]))
            coefs = coefs[3:]
        torch.cuda.synchronize()
        results.append((float(loss.detach()), coefs,
                        {k: v.detach().clone() for k, v in task.state_dict().items() if not k.startswith('input_tensors')}))
    assert results[0][0] == results[1][0]
    assert results[0][1] == results[1][1] and max(results[0][1]) < 1.0     # the clip fired in every replayed step
    for k in results[0][2]:
        assert torch.equal(results[0][2][k], results[1][2][k]), k
