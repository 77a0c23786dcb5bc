"""tests/bn_droppath_ref.py held to plain torch autograd in fp64 on the CPU (out = relu(s * batch_norm(y) + shortcut) and every
gradient), and a plain fp32 run of the same formulas in the kernels' summation order against its bounds: inside half of each on
reals, the rounded fp64 value bit for bit on the integer operands."""
import pytest
import torch

import bn_droppath_ref as D
import bn_ref as B
from helpers import unpack_bits

CPU_SHAPES = [s for s in D.SHAPES if s[0] * s[1] * s[2] <= 1 << 20]


def _close(a, b, what, tol=1e-11):
    err = float((a - b).abs().max() / (1.0 + b.abs().max()))
    assert err < tol, f'{what}: {err:.3e}'


@pytest.mark.parametrize('n,rps,c', [(3, 5, 16), (4, 49, 24), (5, 257, 8)])      # (training BatchNorm: more than one row)
@pytest.mark.parametrize('mode', ['mixed', 'one_dropped', 'zeros'])
def test_reference_is_what_autograd_differentiates(n, rps, c, mode):
    d = D.inputs(n, rps, c, False, seed=3, mode=mode)
    g = torch.Generator().manual_seed(n * rps + c)
    gamma, beta = 1.0 + 0.3 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)
    ag = D.autograd_fp64(d, gamma, beta)
    d = dict(d, scale=ag['scale'], shift=ag['shift'], mean=ag['mean'], rstd=ag['rstd'], coef=torch.zeros(3, c, dtype=torch.float64))
    ref = D.DropRef(d)
    _close(ref.out, ag['out'], 'out')
    s1, s2 = ref.bwd(ref.pattern, 0)['sums']
    m = n * rps
    c1 = gamma.double() * ag['rstd']
    c2 = -c1 * ag['rstd'] * s2 / m
    d['coef'] = torch.stack([c1, c2, -c1 * s1 / m - c2 * ag['mean']])       # what tok_bn_bwd_finalize makes of the two sums
    b = ref.bwd(ref.pattern, 0)
    _close(b['dy'], ag['dy'], 'dy')
    _close(b['ds'], ag['ds'], 'dshortcut')
    _close(s2, ag['dgamma'], 'dgamma')
    _close(s1, ag['dbeta'], 'dbeta')
    dropped = (ref.s == 0).expand_as(b['dy'])
    if bool(dropped.any()):
        # a dropped sample still receives the batch-statistics terms, and they are not zero
        assert torch.equal(b['dy'][dropped], b['dy_dropped'][dropped])
        if mode != 'zeros':
            assert float(b['dy'][dropped].abs().max()) > 0
        assert torch.equal(b['ds'][dropped], b['dt'][dropped])
        assert torch.equal(ref.out[dropped], d['shortcut'].double().clamp_min(0)[dropped])
    if mode == 'zeros':
        assert float(b['sums'].abs().max()) == 0.0


@pytest.mark.parametrize('n,rps,c', CPU_SHAPES)
@pytest.mark.parametrize('integer', [True, False])
def test_fp32_run_against_the_bounds(n, rps, c, integer):
    m = n * rps
    for mode in ('mixed', 'one_dropped'):
        d = D.inputs(n, rps, c, integer, mode=mode)
        ref = D.DropRef(d)
        assert torch.equal(unpack_bits(ref.mask_bytes, m, c), ref.pattern)
        for acc in (0, 1):
            b = ref.bwd(ref.pattern, acc)
            f = D.fp32_run(d, ref.pattern, acc)
            if integer:
                D.assert_exact(d, b)
                D.check_out(None, ref, B.bf(f['out']), True)
                D.check_sums(None, f['sums'], b, m, c, True)
                D.check_apply(None, b, B.bf(f['dy']), B.bf(f['ds']), acc, True)
            else:
                D.check_out(None, ref, f['out'], False, frac=0.5)
                D.check_sums(None, f['sums'], b, m, c, False, frac=0.5)
                D.check_apply(None, b, f['dy'], f['ds'] if acc else f['ds'].double(), acc, False, frac=0.5)


def test_scale_draws_cover_their_sets():
    for integer, vals in ((True, D.S_INT), (False, D.S_REAL)):
        s = D.draw_scale(7, integer)
        assert sorted(set(s.tolist())) == sorted(torch.tensor(vals, dtype=torch.float32).tolist())
        assert float(D.draw_scale(5, integer, mode='one_dropped')[2]) == 0.0
