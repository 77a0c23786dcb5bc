"""The references and bounds of tests/unit3_clip_ref.py, on a CPU:
  * gram_finalize_ref and bn3_prepare_ref equal fp64 autograd of relu(batch_norm(z Wq^T) + shortcut) (F.batch_norm's own running
    statistics included), and d(input) = dz wa + z wb + cvec holds;
  * the clip references equal torch.nn.utils.clip_grad_norm_ / clip_grad_value_;
  * on every input of tests/test_unit3_contract_gpu.py every bound is small against the value (the caps are stated below as
    conditions; the exceptions are named), so no bound can be met trivially;
  * the generic statistics path in the kernels' own precision (fp32 chain for T, fp64 after it) stays inside its bound;
  * deliberately wrong restatements do NOT pass."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import BF, U32
import unit3_clip_ref as M

F64 = torch.float64
TOL = dict(rtol=1e-9, atol=1e-11)


def rejected(what, wrong, out):
    with pytest.raises(AssertionError):
        M.check(None, what, wrong, out.ref, out.bound)


def _unit(m, p, k, seed, rows=5):
    """a real unit in fp64 and the operands of both entries formed from it WITHOUT rounding (so the references are exact algebra)"""
    g = M.gen(seed)
    z = torch.randn(m, p, generator=g, dtype=F64) + 0.2
    w = (torch.randn(k, p, generator=g, dtype=F64) * p ** -0.5).to(BF).double()
    gamma, beta = torch.randn(k, generator=g, dtype=F64) + 1, torch.randn(k, generator=g, dtype=F64)
    sc, gout = torch.randn(m, k, generator=g, dtype=F64), torch.randn(m, k, generator=g, dtype=F64)
    return z, w, gamma, beta, sc, gout


@pytest.mark.parametrize('m,p,k', [(40, 24, 16), (7, 64, 8), (2, 9, 8)])
def test_gram_reference_is_batch_norm(m, p, k):
    z, w, gamma, beta, _, _ = _unit(m, p, k, 1)
    eps, mom = 2.0 ** -16, 0.125
    rm, rv = torch.randn(k, dtype=F64), torch.rand(k, dtype=F64) + 0.5
    d = dict(p=p, k=k, count=m, Z=z.t() @ z, zsum=z.sum(0), w=w, gamma=gamma, beta=beta, rm=rm, rv=rv)
    r = M.gram_finalize_ref(d, momentum=mom, eps=eps)
    y = z @ w.t()
    trm, trv = rm.clone(), rv.clone()
    out = F.batch_norm(y, trm, trv, gamma, beta, True, mom, eps)
    torch.testing.assert_close(r['mean'].ref, y.mean(0), **TOL)
    torch.testing.assert_close(r['var'].ref, y.var(0, unbiased=False), **TOL)
    torch.testing.assert_close(y * r['scale'].ref + r['shift'].ref, out, **TOL)
    torch.testing.assert_close(r['rm'].ref, trm, **TOL)
    torch.testing.assert_close(r['rv'].ref, trv, **TOL)
    torch.testing.assert_close(r['wz'].ref, w @ (z.t() @ z), **TOL)
    # count = 1: the unbiased factor is 1
    d1 = dict(d, count=1, Z=torch.outer(z[0], z[0]), zsum=z[0].clone())
    r1 = M.gram_finalize_ref(d1, momentum=mom, eps=eps)
    torch.testing.assert_close(r1['rv'].ref, (1 - mom) * rv + mom * r1['var'].ref, **TOL)
    assert float(r1['var'].ref.abs().max()) < 1e-12


@pytest.mark.parametrize('m,p,k', [(40, 24, 16), (33, 64, 8), (12, 9, 8)])
def test_prepare_reference_is_autograd(m, p, k):
    z, w, gamma, beta, sc, gout = _unit(m, p, k, 2)
    a = M.unit_autograd(z, w, gamma, beta, sc, gout)
    dz, rows = a['dz'], 5
    wt = torch.arange(1, rows + 1, dtype=F64) / 15
    partial = torch.zeros(2, rows, k, dtype=F64)
    partial[0] = wt[:, None] * dz.sum(0)[None, :]
    Z = z.t() @ z
    d = dict(p=p, k=k, rows=rows, count=m, G=dz.t() @ z, w=w, wz=w @ Z, zsum=z.sum(0), partial=partial, mean=a['mean'],
             rstd=1.0 / torch.sqrt(a['var'] + M.f32(M.EPS)), gamma=gamma,
             prior={n: torch.randn(s, dtype=F64) for n, s in (('dgamma', (k,)), ('dbeta', (k,)), ('dw', (k, p)))})
    a = M.unit_autograd(z, w, gamma, beta, sc, gout, eps=M.f32(M.EPS))
    r = M.bn3_prepare_ref(d)
    for n in ('dgamma', 'dbeta', 'dw'):
        torch.testing.assert_close(r[n].ref, a[n], **TOL)
    dx = dz @ r['wa'].ref.t() + z @ r['wb'].ref + r['cvec'].ref
    torch.testing.assert_close(dx, a['dx'], **TOL)
    c1, c2, c3 = r['coef'].ref
    torch.testing.assert_close(dx, (c1 * dz + c2 * (z @ w.t()) + c3) @ w, **TOL)
    racc = M.bn3_prepare_ref(d, 1, 1)
    for n in ('dgamma', 'dbeta', 'dw'):
        torch.testing.assert_close(racc[n].ref, a[n] + d['prior'][n], **TOL)


def _scale(t):
    return float(t.abs().max())


@pytest.mark.parametrize('p,k', M.GRAM_CASES)
def test_gram_bounds_are_small(p, k):
    """Conditions on the inputs: fp64 folds cast to fp32 (mean; rstd of the block path) are bounded within CAP_ULP = 8 ulps of the
    value (CAP_SMALL_COUNT = 2^-18 at count <= 2, where they stand against eps alone); everything that passes through an fp32
    chain (the generic path's rstd included) within CAP_F32 = 2^-6 of the value or, where
    values cross zero, of the tensor's scale.  The all-zero filter row has var = 0 exactly on both paths."""
    for count in M.COUNTS:
        eps = M.count_eps(p, count)
        d = M.make_gram(p, k, count)
        r = M.gram_finalize_ref(d, eps=eps)
        assert float((r['mean'].bound / r['mean'].ref.abs().clamp_min(1e-30))[r['mean'].ref != 0].max()) < M.CAP_ULP
        rel = r['rstd'].bound / r['rstd'].ref
        cap = M.CAP_F32 if not M.is_block(p) else M.CAP_ULP if count > 2 else M.CAP_SMALL_COUNT
        assert float(rel.max()) < cap, (count, float(rel.max()))
        assert float(r['var'].ref[1]) == 0 and float(r['var'].bound[1]) == 0          # the zero filter row
        assert abs(float(r['rstd'].ref[1]) - 1.0 / np.sqrt(np.float64(np.float32(eps)))) < 1e-13
        for n in ('wz', 'rm', 'rv', 'scale', 'shift'):
            assert float(r[n].bound.max()) < M.CAP_F32 * _scale(r[n].ref), (n, count)


@pytest.mark.parametrize('p,k', M.ONE_COUNT_CASES)
def test_one_count_input_shows_the_unbiased_factor(p, k):
    """count = 1 on operands of non-zero variance at eps = 1e-5: the caps of the other inputs hold, and the running variance with the
    factor of count = 2 (or any other) is rejected"""
    d = M.make_gram_one_count(p, k)
    r = M.gram_finalize_ref(d)
    var = r['var'].ref
    assert float(var[var > 0].min()) > 1.0                                       # nowhere near eps
    rel = r['rstd'].bound / r['rstd'].ref
    assert float(rel.max()) < (M.CAP_ULP if M.is_block(p) else M.CAP_F32)
    for n in ('wz', 'rm', 'rv', 'scale', 'shift'):
        assert float(r[n].bound.max()) < M.CAP_F32 * _scale(r[n].ref), n
    one = M.f32(np.float32(1.0) - np.float32(M.MOMENTUM))
    rejected('rv with the factor 2', one * d['rv'].double() + M.f32(M.MOMENTUM) * 2.0 * var, r['rv'])


@pytest.mark.parametrize('m,p,k', M.CHAIN_CASES)
def test_chain_bounds_are_small(m, p, k):
    """the chain's bounds against the tensors' scale (CAP_CHAIN for d(input): bf16 roundings of terms that cancel; CAP_F32 for the
    fp32 outputs); a data gradient that reads wa as [k][p], or wb's bias dropped, is rejected"""
    c = M.make_chain(m, p, k)
    o = c['out']
    assert float(o['dx'].bound.max()) < M.CAP_CHAIN * _scale(o['dx'].ref)
    for n in ('dw', 'dgamma', 'dbeta'):
        assert float(o[n].bound.max()) < M.CAP_F32 * _scale(o[n].ref), n
    dz, z = c['dz'].double(), c['z'].double()
    torch.testing.assert_close(dz @ c['wa'].t() + z @ c['wb'] + c['cvec'], o['dx'].ref, **TOL)
    rejected('wa read as [k][p]', dz @ c['wa'].reshape(k, p) + z @ c['wb'] + c['cvec'], o['dx'])
    rejected('cvec dropped', dz @ c['wa'].t() + z @ c['wb'], o['dx'])
    rejected('G transposed into dw', o['dw'].ref.t().reshape(k, p), o['dw'])


@pytest.mark.parametrize('p,k', M.PREP_CASES)
def test_prepare_bounds_are_small(p, k):
    """dbeta, dgamma: 8 ulps of the value's scale; coef, dw, wb, cvec: 2^-6 of the tensor's scale (c3, dw and cvec are differences
    of terms that cancel, so the cap is on the scale, not on each element); wa: one bf16 rounding of each element"""
    for acc in (0, 1):
        d = M.make_prepare(p, k, rows=3)
        r = M.bn3_prepare_ref(d, acc, acc)
        for n in ('dgamma', 'dbeta'):
            assert float(r[n].bound.max()) < M.CAP_ULP * _scale(r[n].ref), n
        for n in ('dw', 'wb', 'cvec'):
            assert float(r[n].bound.max()) < M.CAP_F32 * _scale(r[n].ref), n
        for i in range(3):
            assert float(r['coef'].bound[i].max()) < M.CAP_F32 * _scale(r['coef'].ref[i]), i
        nz = r['wa'].ref != 0
        assert float((r['wa'].bound[nz] / r['wa'].ref[nz].abs()).max()) < 2.0 ** -7


@pytest.mark.parametrize('rows', M.ROWS_CASES)
def test_partial_rows_are_distinct(rows):
    d = M.make_prepare(64, 8, rows=rows)
    part = d['partial'][0]
    assert rows == 1 or float((part[1:] - part[:-1]).abs().min(0).values.max()) > 0
    r = M.bn3_prepare_ref(d)
    # a row skipped or counted twice moves dbeta by far more than its bound (the smallest row carries 1 / sum(1..rows) of it)
    if rows > 1:
        for wrong in (part[1:].double().sum(0), part.double().sum(0) + part[-1].double()):
            rejected('dbeta', wrong, r['dbeta'])
    assert M.fold_form(rows) == (4 if rows <= 256 else 8 if rows <= 512 else 16)


@pytest.mark.parametrize('p,k', M.GRAM_GENERIC)
def test_generic_path_in_kernel_order_meets_its_bound(p, k):
    k = min(k, 64)
    d = M.make_gram(p, k, 5000)
    d = {n: (v[:k] if torch.is_tensor(v) and v.shape[:1] == (d['k'],) else v) for n, v in d.items()}
    d['k'] = k
    r = M.gram_finalize_ref(d)
    T, var, rstd = M.gram_kernel_order(d)
    M.check(None, 'wz', T, *r['wz'])
    M.check(None, 'var', var, *r['var'])
    M.check(None, 'rstd', rstd, *r['rstd'])


def test_large_mean_input():
    """the block path's bound rejects the uncentred variance on the large-mean input; the generic path's bound is the measured one
    (large_mean_rstd), small against the value on this input maker too; both references are within 2e-3 of the variance of the rows
    themselves (the fp32 Z)"""
    for p in M.LARGE_P:
        d = M.make_large_mean(p)
        r = M.large_mean_rstd(d)
        want = 1.0 / torch.sqrt(d['var_true'] + M.EPS)
        assert float((r.ref - want).norm() / want.norm()) < 2e-3
        assert float((r.bound / r.ref).max()) < (M.CAP_ULP if M.is_block(p) else M.CAP_F32)
        g = M.gram_finalize_ref(d)
        for n in ('mean', 'wz'):
            assert float(g[n].bound.max()) < M.CAP_F32 * _scale(g[n].ref), n
        _, _, rs = M.gram_kernel_order(d)
        if M.is_block(p):
            rejected('rstd', rs, r)
            M.check(None, 'rstd', M.gram_kernel_order(d, centred=True)[2], *r)
        else:
            M.check(None, 'rstd', rs, *r)
            rejected('rstd 1 % off', rs.double() * 1.01, r)
        assert float((rs.double() - want).norm() / want.norm()) < 5e-2


def test_wrong_restatements_are_rejected():
    d = M.make_prepare(72, 40, rows=65)
    r = M.bn3_prepare_ref(d)
    c1, c2, c3 = r['coef'].ref
    rejected('dw without c3 colsum(z)', c1[:, None] * d['G'].double() + c2[:, None] * d['wz'].double(), r['dw'])
    rejected('wa transposed', r['wa'].ref.t().reshape(72, 40), r['wa'])
    rejected('c3 with the wrong sign of c2 mean', torch.stack([c1, c2, c3 + 2 * c2 * d['mean'].double()]), r['coef'])
    g = M.make_gram(72, 40, 1)
    rg = M.gram_finalize_ref(g)
    rejected('unbiased factor at count = 1', 0.9 * g['rv'].double() + 0.1 * rg['var'].ref * 2 + 1e-3, rg['rv'])
    vals = M.make_spans(M.SPAN_LISTS['cut_in_group'])
    ref, bnd = M.grad_partials_ref(vals)
    wrong, _ = M.grad_partials_ref(vals, shift=1)
    with pytest.raises(AssertionError):
        M.check(None, 'partials', wrong, ref, bnd)


# ---- gradient clip ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n in M.SPAN_LISTS if n not in ('cap', 'over_cap')])
def test_clip_references_are_torch(name):
    numels = M.SPAN_LISTS[name]
    vals = M.make_spans(numels)
    total = sum(numels)
    part, bnd = M.grad_partials_ref(vals)
    assert part.numel() == M.clip_grid(total) and M.clip_chunk(total) * M.clip_grid(total) >= total
    exact = M.math_norm(vals)
    assert abs(float(part.sum()) - exact ** 2) <= float(bnd.sum()) + 1e-300
    assert float((bnd / part.clamp_min(1e-300)).max()) < 2.0 ** -40              # a few fp64 ulps per addition of the chain
    for max_norm in (0.5 * exact, 2.0 * exact):
        ps = [torch.nn.Parameter(v.clone()) for v in vals]
        for q, v in zip(ps, vals):
            q.grad = v.clone()
        tn = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        tot, coef = M.clip_coef_f32(part.numpy(), max_norm)
        assert abs(float(tot) - float(tn)) <= 8 * U32 * exact
        assert abs(float(tot) - exact) <= 1.01 * U32 * exact
        assert (float(coef) == 1.0) == (max_norm > exact)
        for q, s in zip(ps, M.grad_scale_ref(vals, coef)):
            assert float((q.grad.double() - s.double()).abs().max()) <= 8 * U32 * float(s.abs().max())
    assert all(M.same_bits(a, b) for a, b in zip(M.grad_scale_ref(vals, 1.0), vals))


def test_clip_coef_edges():
    tot, c = M.clip_coef_f32(np.zeros(3), 0.5)
    assert tot == 0 and c == 1.0                                                # 0.5 / 1e-6 clamps to 1
    tot, c = M.clip_coef_f32(np.zeros(3), 1e-7)
    assert tot == 0 and c == np.float32(1e-7) / np.float32(1e-6)
    tot, c = M.clip_coef_f32(np.array([1e80, 1e80]), 1.0)
    assert np.isinf(tot) and c == 0
    tot, c = M.clip_coef_f32(np.array([1.0, np.nan]), 1.0)
    assert np.isnan(tot) and np.isnan(c)
    p = np.random.default_rng(0).random(1024) * 1e3
    assert abs(M.fold_kernel_order(p) - float(np.sum(p))) <= 16 * M.U64 * float(np.sum(p))


CLAMP_SPECIALS = [float('inf'), float('-inf'), 0.0, -0.0, float('nan'), 1e-3, -1e-3, 2.0, -2.0, 1e-45, -1e-45]


@pytest.mark.parametrize('v', [1e-3, 0.0, -1.0, float('inf')])
def test_clamp_restatement_is_torch_clamp(v):
    x = torch.cat([torch.tensor(CLAMP_SPECIALS), torch.randn(500, generator=M.gen(5)) * 2e-3])
    want, = M.grad_clamp_ref([x], v)
    mine = M.clamp_ref(x, v)
    nan = torch.isnan(x)
    assert bool(torch.isnan(want[nan]).all()) and M.same_bits(mine[nan], x[nan])     # a NaN keeps its own bits
    assert M.same_bits(mine[~nan], want[~nan])
    ps = [torch.nn.Parameter(x.clone())]
    ps[0].grad = x.clone()
    if v >= 0:
        torch.nn.utils.clip_grad_value_(ps, v)
        assert M.same_bits(ps[0].grad[~nan], want[~nan])


def test_launcher_restatements():
    assert M.split_slices(72, 1032) == (16, 80, 3)            # three trailing slices hold no element
    assert all(M.split_slices(p, k)[2] == 0 for p, k in M.PREP_CASES if (p, k) != (72, 1032))
    assert [M.clip_grid(t) for t in (1, 8192, 8193, 16384, 16385, 1024 * 8192, 1024 * 8192 + 5)] == [1, 1, 2, 2, 3, 1024, 1024]
    assert M.clip_chunk(8193) == 4097 and M.clip_chunk(1024 * 8192 + 5) == 8193
    assert sum(M.SPAN_LISTS['t8193']) == 8193 and sum(M.SPAN_LISTS['t16384']) == 16384 and sum(M.SPAN_LISTS['t16385']) == 16385
    assert sum(M.SPAN_LISTS['over_cap']) == 1024 * 8192 + 5
