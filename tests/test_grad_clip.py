"""Gradient clipping of the fused arena optimizers (torchok_amd.optim.clip_grad_norm_ / clip_grad_value_) and the trainer's
`gradient_clip_val` / `gradient_clip_algorithm` (reference constructor/config_structure.py:161-162), on the host-memory
stand-in of the library: the four clip entry points are written here in torch, over the same span table the kernels read."""
import ctypes
import os

import pytest
import torch

import fake_backend as fb
import torchok_amd as T
from helpers import rel_err
from torchok_amd.optim import clip_grad_norm_, clip_grad_value_

RECIPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'recipes')


def _f64(addr, n):
    return torch.frombuffer((ctypes.c_char * (8 * n)).from_address(int(addr)), dtype=torch.float64, count=n)


class ClipFake(fb.FakeTok):
    """FakeTok plus tok_grad_sqnorm_partial / tok_grad_clip_coef / tok_grad_scale / tok_grad_clamp."""

    @staticmethod
    def _spans(spans, n):
        tbl = fb._t(spans, (n, 3), torch.int64)
        start = 0
        for ptr_, numel, st in tbl.tolist():
            assert st == start and numel >= 1 and ptr_ % 16 == 0
            start += numel
            yield fb._t(ptr_, (numel,), torch.float32)

    def tok_grad_sqnorm_partial(self, spans, n, total, partials, st):
        self.calls.append('grad_sqnorm_partial')
        acc = sum(float((g.double() ** 2).sum()) for g in self._spans(spans, n))
        out = _f64(partials, T._C.TOK_GRAD_CLIP_MAX_PARTIALS)
        out.zero_()
        out[0] = acc
        return 0

    def tok_grad_clip_coef(self, partials, total, max_norm, total_norm, coef, st):
        self.calls.append('grad_clip_coef')
        tot = torch.tensor(float(_f64(partials, T._C.TOK_GRAD_CLIP_MAX_PARTIALS).sum()) ** 0.5,
                           dtype=torch.float32)
        fb._t(total_norm, (1,), torch.float32)[0] = tot
        fb._t(coef, (1,), torch.float32)[0] = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (tot + 1e-6), max=1.0)
        return 0

    def tok_grad_scale(self, spans, n, total, coef, st):
        self.calls.append('grad_scale')
        c = fb._t(coef, (1,), torch.float32)[0].clone()
        if c != 1.0:
            for g in self._spans(spans, n):
                g.mul_(c)
        return 0

    def tok_grad_clamp(self, spans, n, total, v, st):
        self.calls.append('grad_clamp')
        for g in self._spans(spans, n):
            g.clamp_(-v, v)
        return 0


@pytest.fixture
def clip_backend():
    token = fb.install(ClipFake())
    yield token[0]
    fb.uninstall(token)


def _params(seed, shapes=((6, 5), (5,), (4, 3, 3, 3), (7,), (1,), (65,))):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]


def _grads(step, params, scale):
    g = torch.Generator().manual_seed(1000 + step)
    return [torch.randn(p.shape, generator=g) * scale for p in params]


CASES = [('SGD', torch.optim.SGD, dict(lr=0.1, momentum=0.9, weight_decay=1e-4)),
         ('SGD', torch.optim.SGD, dict(lr=0.1, momentum=0.9, nesterov=True)),
         ('Adam', torch.optim.Adam, dict(lr=1e-2)),
         ('AdamW', torch.optim.AdamW, dict(lr=1e-2, weight_decay=0.05)),
         ('RMSprop', torch.optim.RMSprop, dict(lr=1e-2, momentum=0.5, centered=True))]
SCALES = (0.1, 3.0, 0.05)      # gradient sizes of the 3 steps: the norm clips in the middle step only (max_norm 2)


def _groups(params):
    return [{'params': params[:3]}, {'params': params[3:], 'lr': 0.05}]


@pytest.mark.parametrize('name,tcls,kw', CASES)
def test_clip_grad_norm_equals_torch(clip_backend, name, tcls, kw):
    ours_p, ref_p = _params(0), _params(0)
    ours, ref = T.OPTIMIZERS.get(name)(_groups(ours_p), **kw), tcls(_groups(ref_p), **kw)
    clipped = []
    for step, scale in enumerate(SCALES):
        for ps in (ours_p, ref_p):
            for p, g in zip(ps, _grads(step, ps, scale)):
                p.grad = g.clone()
        n_ours = clip_grad_norm_(ours, 2.0)
        n_ref = torch.nn.utils.clip_grad_norm_(ref_p, 2.0)
        assert n_ours.dim() == 0 and n_ours.dtype == torch.float32
        assert abs(float(n_ours) - float(n_ref)) <= 2e-5 * float(n_ref), (step, float(n_ours), float(n_ref))
        clipped.append(float(n_ref) > 2.0)
        for a, b in zip(ours_p, ref_p):
            assert rel_err(a.grad, b.grad) < 2e-5
        ours.step()
        ref.step()
        for a, b in zip(ours_p, ref_p):
            assert rel_err(a, b) < 2e-5, (name, kw, step)
    assert clipped == [False, True, False]


@pytest.mark.parametrize('name,tcls,kw', CASES)
def test_clip_grad_value_equals_torch(clip_backend, name, tcls, kw):
    ours_p, ref_p = _params(1), _params(1)
    ours, ref = T.OPTIMIZERS.get(name)(_groups(ours_p), **kw), tcls(_groups(ref_p), **kw)
    for step, scale in enumerate(SCALES):
        for ps in (ours_p, ref_p):
            for p, g in zip(ps, _grads(step, ps, scale)):
                p.grad = g.clone()
        assert clip_grad_value_(ours, 0.5) is None
        torch.nn.utils.clip_grad_value_(ref_p, 0.5)
        for a, b in zip(ours_p, ref_p):
            assert torch.equal(a.grad, b.grad)
        ours.step()
        ref.step()
        for a, b in zip(ours_p, ref_p):
            assert rel_err(a, b) < 2e-5, (name, kw, step)


def test_stale_slot_is_skipped(clip_backend):
    """zero_grad() leaves the gradient arena as it was: a parameter without a gradient this step still has large values in
    its slot.  torch skips that parameter; so must the norm, the scale and the update."""
    ours_p, ref_p = _params(2), _params(2)
    ours, ref = T.OPTIMIZERS.get('SGD')(_groups(ours_p), lr=0.1, momentum=0.9), \
        torch.optim.SGD(_groups(ref_p), lr=0.1, momentum=0.9)
    for ps, opt in ((ours_p, ours), (ref_p, ref)):
        for p, g in zip(ps, _grads(0, ps, 100.0)):
            p.grad = g.clone()
        opt.step()
        opt.zero_grad(set_to_none=True)
    skip = 2
    slot = ours._arenas[0].grad_view(skip)
    assert slot.abs().max() > 10                       # the stale slot really holds last step's large values
    before = slot.clone()
    for ps in (ours_p, ref_p):
        for i, (p, g) in enumerate(zip(ps, _grads(1, ps, 0.5))):
            p.grad = None if i == skip else g.clone()
    n_ours, n_ref = clip_grad_norm_(ours, 1.0), torch.nn.utils.clip_grad_norm_(ref_p, 1.0)
    assert abs(float(n_ours) - float(n_ref)) <= 2e-5 * float(n_ref) and float(n_ref) > 1.0
    assert torch.equal(slot, before)                   # neither read nor scaled
    ours.step()
    ref.step()
    for a, b in zip(ours_p, ref_p):
        assert rel_err(a, b) < 2e-5


def test_foreign_grads_are_adopted_and_table_is_cached(clip_backend):
    ps = _params(3)
    opt = T.OPTIMIZERS.get('SGD')(ps, lr=0.1)
    for step in range(3):
        for p, g in zip(ps, _grads(step, ps, 1.0)):
            p.grad = g.clone()                        # stand-alone tensors, as plain autograd leaves them
        clip_grad_norm_(opt, 1.0)
        arena = opt._arenas[0]
        assert all(p.grad.data_ptr() == arena.grad_view(i).data_ptr() for i, p in enumerate(ps))   # moved into the slots
        if step == 0:
            table = opt._clip_state.table
        assert opt._clip_state.table is table         # same pattern: no new upload
        opt.step()
    ps[1].grad = None
    ps[0].grad = torch.ones_like(ps[0])
    clip_grad_norm_(opt, 1e9)
    assert opt._clip_state.table is not table and opt._clip_state.n == len(ps) - 1


def test_edge_cases(clip_backend):
    ps = _params(4)
    opt = T.OPTIMIZERS.get('AdamW')(ps, lr=1e-3)
    n = clip_grad_norm_(opt, 1.0)                      # no gradients at all: zero, no launch
    assert float(n) == 0.0 and 'grad_sqnorm_partial' not in clip_backend.calls
    with pytest.raises(NotImplementedError):
        clip_grad_norm_(opt, 1.0, norm_type=1.0)
    with pytest.raises(NotImplementedError):
        clip_grad_norm_(opt, 1.0, norm_type='inf')
    with pytest.raises(TypeError, match='torch.nn.utils'):
        clip_grad_norm_(ps, 1.0)
    with pytest.raises(TypeError, match='torch.nn.utils'):
        clip_grad_value_(iter(ps), 1.0)
    for p in ps:
        p.grad = torch.ones_like(p)
    ps[0].grad[0, 0] = float('nan')
    with pytest.raises(RuntimeError, match='non-finite'):
        clip_grad_norm_(opt, 1.0, error_if_nonfinite=True)
    assert clip_backend.calls[-1] == 'grad_clip_coef'  # raised before scaling, as torch
    n = clip_grad_norm_(opt, 1.0)
    assert torch.isnan(n) and all(torch.isnan(p.grad).all() for p in ps)


def test_clip_norm_returns_a_fresh_tensor(clip_backend):
    ps = _params(5)
    opt = T.OPTIMIZERS.get('SGD')(ps, lr=0.1)
    norms = []
    for step in range(2):
        for p, g in zip(ps, _grads(step, ps, 1.0 + step)):
            p.grad = g.clone()
        norms.append(clip_grad_norm_(opt, 1e9))
    assert float(norms[0]) != float(norms[1])


# ---- the trainer options ----------------------------------------------------------------------------------------------------
def test_resolve_gradient_clip():
    from torchok_amd.run import resolve_gradient_clip, resolve_strategy
    assert resolve_strategy({'gradient_clip_val': 35, 'gradient_clip_algorithm': 'norm'})[:2] == (False, 1)
    assert resolve_gradient_clip({}) is None
    assert resolve_gradient_clip({'gradient_clip_val': 35}) == ('norm', 35.0)          # norm when the algorithm is unset
    assert resolve_gradient_clip({'gradient_clip_val': 0.5, 'gradient_clip_algorithm': 'Value'}) == ('value', 0.5)
    assert resolve_gradient_clip({'gradient_clip_val': 1, 'gradient_clip_algorithm': 'NORM'}) == ('norm', 1.0)
    assert resolve_gradient_clip({'gradient_clip_val': 0}) is None                     # Lightning: clip_val <= 0 is off
    assert resolve_gradient_clip({'gradient_clip_val': -1.0, 'gradient_clip_algorithm': 'value'}) is None
    assert resolve_gradient_clip({'gradient_clip_val': None, 'gradient_clip_algorithm': 'norm'}) is None
    with pytest.raises(ValueError, match='gradient_clip_algorithm'):
        resolve_gradient_clip({'gradient_clip_val': 1.0, 'gradient_clip_algorithm': 'l1'})
    for key, val in (('accumulate_grad_batches', 2), ('sync_batchnorm', True)):
        with pytest.raises(NotImplementedError):
            resolve_strategy({key: val})


def _fit(overrides, steps=2):
    from torchok_amd.run import fit
    os.environ.setdefault('HOME', '/root')
    cfg = T.load_config(os.path.join(RECIPES, 'classification_cifar10_multi_validation.yaml'),
                        overrides=dict({'task.params.backbone_params.pretrained': False, 'trainer.precision': 'bf16',
                                        'trainer.devices': 1}, **overrides))
    torch.manual_seed(0)
    batches = [{'image': torch.randn(4, 3, 32, 32), 'target': torch.randint(0, 10, (4,))} for _ in range(steps)]
    return fit(cfg, batches=batches, max_steps=steps, device='cpu')


@pytest.mark.parametrize('algo', [None, 'norm', 'value'])
def test_shipped_recipe_with_gradient_clip_runs_through_fit(clip_backend, algo):
    ov = {'trainer.gradient_clip_val': 0.5}
    if algo is not None:
        ov['trainer.gradient_clip_algorithm'] = algo
    res = _fit(ov)
    assert res['steps'] == 2
    want = 'grad_clamp' if algo == 'value' else 'grad_scale'
    assert clip_backend.calls.count(want) == 2
    # the clip runs between the last backward kernel and the optimizer step of each step
    i = clip_backend.calls.index(want)
    assert not any(c.endswith('_step') for c in clip_backend.calls[:i])
    assert any(c.endswith('_step') for c in clip_backend.calls[i:])


def test_fit_without_clip_launches_no_clip_kernel(clip_backend):
    _fit({'trainer.gradient_clip_val': 0})
    assert not any(c.startswith('grad_') for c in clip_backend.calls)
    with pytest.raises(ValueError, match='gradient_clip_algorithm'):
        _fit({'trainer.gradient_clip_val': 1.0, 'trainer.gradient_clip_algorithm': 'bogus'})
