"""Kernel contract of csrc/optim.hip, element by element against tests/optim_ref.py (fp64 one-step formulas, tied to torch.optim in
float64 by tests/test_optim_ref.py; that module derives every bound from the kernel source).

Every configuration runs six steps with fresh gradients (one element in eight exactly zero).  After every step the parameter
and every state array are compared with the fp64 step applied to the DEVICE's previous state and the float hyper-parameters the
kernel received, so the bound stays a one-step bound; the bf16 shadow must be bit for bit `.to(bfloat16)` of the device's new
parameter.  Every array sits in a helpers.GuardedSpan whose guards are checked after every step.  The count 4096 * 256 + 17 sends
every thread of the capped grid on a second grid-stride trip (asserted).  tok_fill_f32 / tok_scale_f32 are bit exact.

Recorded err / bound above 0.5 (up to 0.99 on `param`, 0.5 - 0.65 on some state arrays): the bounds are tight by construction.
Each is the plain sum of the largest error of every rounding on the path, U32 = 2^-24 being the largest relative error of ONE
fp32 rounding, which is attained.  The parameter's own term |w| carries a single rounding in Adam without decoupled decay and in
RMSprop (the final subtraction), so wherever the update is small next to |w| an exact kernel records up to 1; SGD's first
momentum buffer d = g + wd * w (two roundings counted, one FMA on the device) records 0.5; and where the two or three terms of
an update have the same magnitude and their roundings fall the same way, a state array records 0.5 - 0.9.  A plain IEEE fp32
evaluation of the same formulas on the CPU (torch, no FMA) records the same figures against these bounds — 0.87 for the RMSprop
momentum buffer, 0.55 for grad_avg, 0.9 for the parameter over 257 elements and six steps — so they are the arithmetic's, not
the kernel's.  A result above 1 needs a rounding the source does not contain."""
import pytest
import torch

import optim_ref as R
from helpers import BF, ERR_INVALID, F32, U32, assert_bounded, gin, gout, last_error
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
G = 64
CAP = 4096 * 256
I64 = torch.int64
MOD = 'test_optim_contract_gpu::'


def _run(fn, *args):
    _C.check(getattr(_C.lib(), fn)(*args, stream_ptr()), fn)
    torch.cuda.synchronize()


def _state(count, init=None):
    return gout(count, F32, G, init=(torch.zeros(count) if init is None else init).cuda())


def _compare(arrays, prev_refs, test, what):
    """arrays {name: span}; prev_refs = (new, bound) of the reference step"""
    new, bound = prev_refs
    for name, span in arrays.items():
        if span is None:
            continue
        span.check(f'{what} {name}')
        assert_bounded(span.value(), new[name], bound[name], 0.0, U32, what=f'{what} {name}', test=MOD + test)


def _shadow_is_the_cast(shadow, p, what):
    if shadow is None:
        return
    shadow.check(what + ' shadow')
    assert torch.equal(shadow.value().view(torch.int16), p.value().to(BF).view(torch.int16)), what + ': shadow != bf16(param)'


def _second_trip(count):
    if count == R.COUNTS[3]:
        assert count > CAP                       # grid_for caps the grid at 4096 blocks of 256: a second grid-stride trip


@pytest.mark.parametrize('name,count', R.SGD_CASES, ids=str)
def test_sgd(name, count):
    _second_trip(count)
    cfg = R.SGD_CONFIGS[name]
    c = R.as_f32(cfg)
    w0, grads = R.problem(count, 1)
    p = _state(count, w0)
    buf = _state(count) if cfg['momentum'] != 0 else None                      # momentum-free SGD: a NULL buffer
    shadow = None if name == 'plain' else gout(count, BF, G)                   # a NULL shadow is accepted
    for t in range(R.STEPS):
        g = gin(grads[t], G)
        ref = R.sgd_step(p.value(), grads[t], buf.value() if buf else None, first=(t == 0), **c)
        _run('tok_sgd_step', p.ptr, g.ptr, buf.ptr if buf else None, shadow.ptr if shadow else None, count, c['lr'], c['momentum'],
             c['dampening'], c['weight_decay'], int(c['nesterov']), int(t == 0), int(c['maximize']))
        what = f'{name} count={count} step={t}'
        _compare({'param': p, 'buf': buf}, ref, 'test_sgd', what)
        _shadow_is_the_cast(shadow, p, what)


@pytest.mark.parametrize('capturable', [False, True], ids=['host_step', 'capturable'])
@pytest.mark.parametrize('name,count', R.ADAM_CASES, ids=str)
def test_adam(name, count, capturable):
    _second_trip(count)
    cfg = R.ADAM_CONFIGS[name]
    c = R.as_f32({k: v for k, v in cfg.items() if k != 'step0'})
    w0, grads = R.problem(count, 2)
    p, m, v = _state(count, w0), _state(count), _state(count)
    shadow = None if name == 'adamw_nowd' else gout(count, BF, G)             # the bf16 shadow of Adam; NULL accepted
    step_dev = gout(1, I64, G, init=torch.tensor([cfg['step0'] - 1]).cuda()) if capturable else None
    hyper = (c['lr'], c['beta1'], c['beta2'], c['eps'], c['weight_decay'], int(c['decoupled']))
    for t in range(R.STEPS):
        step = cfg['step0'] + t
        g = gin(grads[t], G)
        w_before = p.value().clone()
        ref = R.adam_step(w_before, grads[t], m.value(), v.value(), step, **c)
        ptrs = (p.ptr, g.ptr, m.ptr, v.ptr, shadow.ptr if shadow else None, count)
        if capturable:
            _run('tok_adam_step_capturable', *ptrs, *hyper, step_dev.ptr, int(c['maximize']))
            step_dev.check('step_dev')
            assert int(step_dev.value()) == step - 1, '*step_dev is read, never written by the step'
            _run('tok_step_advance', step_dev.ptr)
            step_dev.check('step_dev')
            assert int(step_dev.value()) == step, 'tok_step_advance adds exactly 1'
        else:
            _run('tok_adam_step', *ptrs, *hyper, step, int(c['maximize']))
        what = f'{name} count={count} step={step} capturable={capturable}'
        _compare({'param': p, 'm': m, 'v': v}, ref, 'test_adam', what)
        _shadow_is_the_cast(shadow, p, what)
        if t == 0 and cfg['weight_decay'] == 0:        # zero state and an exactly zero gradient: the step is exactly zero
            z = grads[0] == 0
            assert count < 255 or bool(z.any())
            assert torch.equal(p.value()[z].view(torch.int32), w_before[z].view(torch.int32)), what
            assert bool((m.value()[z].view(torch.int32) == 0).all()) and bool((v.value()[z].view(torch.int32) == 0).all()), what


@pytest.mark.parametrize('name,count', R.RMSPROP_CASES, ids=str)
def test_rmsprop(name, count):
    _second_trip(count)
    cfg = R.RMSPROP_CONFIGS[name]
    c = R.as_f32(cfg)
    w0, grads = R.problem(count, 3)
    p, sq = _state(count, w0), _state(count)
    buf = _state(count) if cfg['momentum'] > 0 else None
    ga = _state(count) if cfg['centered'] else None
    for t in range(R.STEPS):
        g = gin(grads[t], G)
        ref = R.rmsprop_step(p.value(), grads[t], sq.value(), buf.value() if buf else None, ga.value() if ga else None, **c)
        if cfg['centered']:
            assert float(R.centered_factor(ref[0]['sq'], ref[0]['ga']).max()) < 100          # the cap the bound was derived under
        _run('tok_rmsprop_step', p.ptr, g.ptr, sq.ptr, buf.ptr if buf else None, ga.ptr if ga else None, count, c['lr'], c['alpha'],
             c['eps'], c['weight_decay'], c['momentum'], int(c['centered']), int(c['maximize']))
        _compare({'param': p, 'sq': sq, 'buf': buf, 'ga': ga}, ref, 'test_rmsprop', f'{name} count={count} step={t}')


@pytest.mark.parametrize('count', R.COUNTS)
def test_fill_and_scale_are_bit_exact(count):
    _second_trip(count)
    x = torch.randn(count, generator=torch.Generator().manual_seed(count))
    for value in (0.1, -3.0, 0.0):
        dst = gout(count, F32, G)
        _run('tok_fill_f32', dst.ptr, value, count)
        dst.check(f'fill count={count}')
        assert torch.equal(dst.value().view(torch.int32), torch.full((count,), value, dtype=F32).view(torch.int32))
    for factor in (0.5, 1.0 / 3.0, -1.7):
        dst = gout(count, F32, G, init=x.cuda())
        _run('tok_scale_f32', dst.ptr, factor, count)
        dst.check(f'scale count={count}')
        assert torch.equal(dst.value().view(torch.int32), (x * torch.tensor(factor, dtype=F32)).view(torch.int32))


def test_refusals():
    """every TOK_CHECK_ARG of optim.hip: the invalid-argument code, the function named in tok_last_error, nothing written"""
    lib, st = _C.lib(), stream_ptr()
    src = gin(torch.zeros(1024), G)
    out, sh = gout(1024, F32, G), gout(1024, BF, G)
    i, o, s = src.ptr, out.ptr, sh.ptr
    sgd = (0.1, 0.9, 0.0, 0.0, 0, 0, 0, st)
    adam = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0)
    rms = (1e-2, 0.99, 1e-8, 0.0)
    calls = [('tok_sgd_step', (None, i, o, s, 8, *sgd)), ('tok_sgd_step', (o, None, o, s, 8, *sgd)), ('tok_sgd_step', (o, i, o, s, 0, *sgd)),
             ('tok_sgd_step', (o, i, None, s, 8, *sgd)),                                              # a momentum with no buffer
             ('tok_adam_step', (None, i, o, o, s, 8, *adam, 1, 0, st)), ('tok_adam_step', (o, None, o, o, s, 8, *adam, 1, 0, st)),
             ('tok_adam_step', (o, i, None, o, s, 8, *adam, 1, 0, st)), ('tok_adam_step', (o, i, o, None, s, 8, *adam, 1, 0, st)),
             ('tok_adam_step', (o, i, o, o, s, 0, *adam, 1, 0, st)), ('tok_adam_step', (o, i, o, o, s, 8, *adam, 0, 0, st)),
             ('tok_adam_step', (o, i, o, o, s, 8, *adam, -3, 0, st)),                                 # step < 1
             ('tok_adam_step_capturable', (None, i, o, o, s, 8, *adam, i, 0, st)),
             ('tok_adam_step_capturable', (o, None, o, o, s, 8, *adam, i, 0, st)),
             ('tok_adam_step_capturable', (o, i, None, o, s, 8, *adam, i, 0, st)),
             ('tok_adam_step_capturable', (o, i, o, None, s, 8, *adam, i, 0, st)),
             ('tok_adam_step_capturable', (o, i, o, o, s, 0, *adam, i, 0, st)),
             ('tok_adam_step_capturable', (o, i, o, o, s, 8, *adam, None, 0, st)),
             ('tok_step_advance', (None, st)),
             ('tok_rmsprop_step', (None, i, o, o, o, 8, *rms, 0.9, 1, 0, st)), ('tok_rmsprop_step', (o, None, o, o, o, 8, *rms, 0.9, 1, 0, st)),
             ('tok_rmsprop_step', (o, i, None, o, o, 8, *rms, 0.9, 1, 0, st)), ('tok_rmsprop_step', (o, i, o, o, o, 0, *rms, 0.9, 1, 0, st)),
             ('tok_rmsprop_step', (o, i, o, None, o, 8, *rms, 0.9, 1, 0, st)),                        # momentum without its buffer
             ('tok_rmsprop_step', (o, i, o, o, None, 8, *rms, 0.0, 1, 0, st)),                        # centered without grad_avg
             ('tok_fill_f32', (None, 1.0, 8, st)), ('tok_fill_f32', (o, 1.0, 0, st)),
             ('tok_scale_f32', (None, 1.0, 8, st)), ('tok_scale_f32', (o, 1.0, 0, st))]
    for fn, args in calls:
        rc = getattr(lib, fn)(*args)
        assert rc == ERR_INVALID and fn + ':' in last_error(), (fn, args[:-1], rc, last_error())
    torch.cuda.synchronize()
    for buf in (out, sh):
        buf.check('refused call')
        assert buf.untouched()
    src.check('refused call')
