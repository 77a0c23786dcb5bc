"""tests/optim_ref.py against torch.optim in float64: six steps of the fp64 formulas equal torch.optim.SGD / Adam / AdamW /
RMSprop to 1e-12 in every array, for every configuration and count tests/test_optim_contract_gpu.py runs, Adam also with
capturable=True; and the gradients keep the cancellation of centred RMSprop below its cap at every step."""
import pytest
import torch

import optim_ref as R

F64 = torch.float64
TOL = dict(rtol=1e-12, atol=1e-12)


def _close(a, b, what):
    assert torch.allclose(a, b, **TOL), (what, float((a - b).abs().max()))


def _param(w0):
    return torch.nn.Parameter(w0.to(F64).clone())


@pytest.mark.parametrize('name,count', R.SGD_CASES, ids=str)
def test_sgd_formula_is_torch(name, count):
    cfg = R.SGD_CONFIGS[name]
    w0, grads = R.problem(count, 1)
    p = _param(w0)
    opt = torch.optim.SGD([p], foreach=False, **cfg)
    w, buf = w0.to(F64), None
    for t in range(R.STEPS):
        p.grad = grads[t].to(F64).clone()
        opt.step()
        new, bound = R.sgd_step(w, grads[t], buf, first=(t == 0), **cfg)
        w, buf = new['param'], new.get('buf')
        _close(w, p.detach(), f'param step {t}')
        if cfg['momentum'] != 0:
            _close(buf, opt.state[p]['momentum_buffer'], f'buf step {t}')
        assert all(bool((b >= 0).all()) for b in bound.values())


@pytest.mark.parametrize('capturable', [False, True])
@pytest.mark.parametrize('name,count', R.ADAM_CASES, ids=str)
def test_adam_formula_is_torch(name, count, capturable, monkeypatch):
    cfg = R.ADAM_CONFIGS[name]
    if capturable:
        # the capturable branch of torch.optim.adam is plain tensor arithmetic; its guard only lists the devices a graph can be
        # captured on.  With the default dtype at float64 its step counter and bias corrections are float64 tensors.
        import torch.optim.adam as A
        import torch.optim.adamw as AW
        devices = A._get_capturable_supported_devices() + ['cpu']
        for mod in (A, AW):
            if hasattr(mod, '_get_capturable_supported_devices'):
                monkeypatch.setattr(mod, '_get_capturable_supported_devices', lambda *a, **k: devices)
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        w0, grads = R.problem(count, 2)
        p = _param(w0)
        cls = torch.optim.AdamW if cfg['decoupled'] else torch.optim.Adam
        opt = cls([p], lr=cfg['lr'], betas=(cfg['beta1'], cfg['beta2']), eps=cfg['eps'], weight_decay=cfg['weight_decay'],
                  maximize=cfg['maximize'], capturable=capturable, foreach=False)
        opt.state[p] = {'step': torch.tensor(float(cfg['step0'] - 1), dtype=F64), 'exp_avg': torch.zeros(count, dtype=F64),
                        'exp_avg_sq': torch.zeros(count, dtype=F64)}
        w, m, v = w0.to(F64), torch.zeros(count, dtype=F64), torch.zeros(count, dtype=F64)
        for t in range(R.STEPS):
            p.grad = grads[t].to(F64).clone()
            opt.step()
            new, bound = R.adam_step(w, grads[t], m, v, cfg['step0'] + t, **{k: c for k, c in cfg.items() if k != 'step0'})
            if t == 0 and cfg['weight_decay'] == 0:          # zero state, zero gradient: the step is exactly zero
                z = grads[0] == 0
                assert torch.equal(new['param'][z], w[z]) and (count < 255 or bool(z.any()))
            w, m, v = new['param'], new['m'], new['v']
            _close(w, p.detach(), f'param step {t}')
            _close(m, opt.state[p]['exp_avg'], f'exp_avg step {t}')
            _close(v, opt.state[p]['exp_avg_sq'], f'exp_avg_sq step {t}')
            assert all(bool((b >= 0).all()) and bool(torch.isfinite(b).all()) for b in bound.values())
        assert float(opt.state[p]['step']) == cfg['step0'] + R.STEPS - 1
    finally:
        torch.set_default_dtype(old)


@pytest.mark.parametrize('name,count', R.RMSPROP_CASES, ids=str)
def test_rmsprop_formula_is_torch(name, count):
    cfg = R.RMSPROP_CONFIGS[name]
    w0, grads = R.problem(count, 3)
    p = _param(w0)
    opt = torch.optim.RMSprop([p], foreach=False, **cfg)
    z = torch.zeros(count, dtype=F64)
    w, sq, buf, ga = w0.to(F64), z, z, z
    worst = 0.0
    for t in range(R.STEPS):
        p.grad = grads[t].to(F64).clone()
        opt.step()
        new, bound = R.rmsprop_step(w, grads[t], sq, buf, ga, **cfg)
        w, sq, buf, ga = new['param'], new['sq'], new.get('buf', z), new.get('ga', z)
        st = opt.state[p]
        _close(w, p.detach(), f'param step {t}')
        _close(sq, st['square_avg'], f'square_avg step {t}')
        if cfg['momentum'] > 0:
            _close(buf, st['momentum_buffer'], f'momentum_buffer step {t}')
        if cfg['centered']:
            _close(ga, st['grad_avg'], f'grad_avg step {t}')
            assert bool((sq - ga * ga >= 0).all())
            worst = max(worst, float(R.centered_factor(sq, ga).max()))
        assert all(bool((b >= 0).all()) and bool(torch.isfinite(b).all()) for b in bound.values())
    assert worst < 100, worst                                  # the conditioning cap of the centred bound


def test_float_hyperparameters_are_not_the_literals():
    """what the header of optim_ref.py says about the C ABI: 1 - float(0.999) is 1.3e-5 away from 1e-3"""
    b2 = R.f32(0.999)
    assert abs((1 - b2) / 1e-3 - 1) > 1e-5 and R.as_f32(dict(a=0.5, n=True, s=3)) == dict(a=0.5, n=True, s=3)
