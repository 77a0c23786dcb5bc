"""The LayerNorm reference and bounds of tests/layernorm_ref.py: the fp64 reference agrees with torch's own layer_norm and with
the fake backend, a plain fp32 run of the same formulas stays inside HALF of every bound of the contract (so an exact fp32
kernel passes tests/test_layernorm_contract_gpu.py), and a one-pass variance E[x^2] - mu^2 does NOT pass the rstd bound."""
import pytest
import torch
import torch.nn.functional as F

from fake_backend import FakeTok
from helpers import assert_bounded
from layernorm_ref import EPS, LNRef, check_bwd, check_fwd, fp32_run, make_inputs

P = lambda t: None if t is None else t.data_ptr()       # noqa: E731
SHAPES = [(rows, c) for c in (8, 100, 128, 136, 264, 520, 1024, 1032) for rows in (1, 5, 33)] + [(4099, 8)]


@pytest.mark.parametrize('rows,c', SHAPES)
def test_fp32_run_stays_inside_half_of_every_bound(rows, c):
    for sc, rs in ((0, 0), (1, 1)):
        d = make_inputs(rows, c, sc, rs, seed=rows + c)
        ref = LNRef(d)
        for acc in (0, 1):
            out, mean, rstd, dx, dg, db = fp32_run(d, ref, acc)
            check_fwd('fp32', ref, out, mean, rstd, frac=0.5)
            check_bwd('fp32', ref, acc, dx, dg, db, frac=0.5)


def test_reference_agrees_with_torch_and_the_fake_backend():
    rows, c = 33, 136
    d = make_inputs(rows, c, 1, 1, seed=1)
    ref = LNRef(d)
    x = d['x'].double().requires_grad_(True)
    ga, be = d['gamma'].double().requires_grad_(True), d['beta'].double().requires_grad_(True)
    sc = d['row_scale'].double().repeat_interleave(d['rps'])[:rows, None]
    y = F.layer_norm(x, (c,), ga, be, EPS) * sc + d['shortcut'].double()
    y.backward(d['dout'].double())
    assert (y.detach() - ref.out).abs().max() < 1e-12
    assert (ga.grad - ref.dgamma).abs().max() < 1e-4 * ref.m_dgamma.max()      # (ref: fp32-rounded statistics)
    assert (be.grad - ref.dbeta).abs().max() < 1e-12 * ref.m_dbeta.max()
    assert (x.grad - ref.dx[0]).abs().max() < 1e-4 * ref.m_dx.max()
    fake = FakeTok()
    out, mean, rstd = torch.empty(rows, c, dtype=torch.bfloat16), torch.empty(rows), torch.empty(rows)
    assert fake.tok_layernorm_fwd(P(d['x']), P(d['shortcut']), P(d['row_scale']), d['rps'], P(d['gamma']), P(d['beta']), P(out),
                                  P(mean), P(rstd), rows, c, c, EPS, None) == 0
    check_fwd('fake', ref, out, mean, rstd)
    assert float(ref.rstd[0]) == EPS ** -0.5 and float(ref.rstd[2]) == EPS ** -0.5        # the constant rows


def test_one_pass_variance_fails_the_rstd_bound():
    d = make_inputs(5, 128, 0, 0, seed=2)
    ref = LNRef(d)
    x = d['x'].float()
    mu = x.mean(1)
    rstd = torch.rsqrt((x * x).mean(1) - mu * mu + EPS)
    with pytest.raises(AssertionError):
        assert_bounded(rstd[1:2], ref.rstd[1:2], ref.b_rstd[1:2], 0.0, 1.0, 'rstd of the offset row')
