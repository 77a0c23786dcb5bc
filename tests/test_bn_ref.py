"""The BatchNorm / stem references and bounds of tests/bn_ref.py: the fp64 reference agrees with torch's own batch_norm autograd
in fp64 (with and without shortcut and ReLU) and with the fake backend within the bounds; a plain fp32 run of the kernels'
formulas stays inside HALF of every bound at every shape of tests/test_bn_contract_gpu.py (the two largest row counts are
replaced by one of 4099 rows), so a correct fp32 kernel passes; the inputs keep the share of elements near z = 0 under 0.1 %;
and wrong variants (a row left out of a sum, biased running variance, c2 and c3 exchanged, the shortcut left out of the ReLU
pattern, an fp32 E[y^2] - mu^2 variance on the large-mean channel) do NOT pass."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref as R
from fake_backend import FakeTok
from helpers import BF, unpack_bits

P = lambda t: None if t is None else t.data_ptr()       # noqa: E731
CPU_STREAM = [s for s in R.STREAM_SHAPES if s[0] < 70000] + [(4099, 8)]
CONFIGS = [(1, 1, 1, 1), (1, 0, 1, 0), (1, 0, 0, 0), (0, 0, 0, 0), (0, 1, 0, 1)]        # relu, shortcut, mask given, ds_acc


@pytest.mark.parametrize('m,c', CPU_STREAM)
def test_fp32_run_of_the_streaming_kernels_stays_inside_half_of_every_bound(m, c):
    for integer in (True, False):
        d = R.stream_inputs(m, c, integer)
        for relu, with_sc, use_mask, acc in CONFIGS:
            ref = R.StreamRef(d, relu, with_sc)
            b = ref.bwd(use_mask, acc)
            if integer:
                R.assert_exact_sums(ref, b)
            f = R.fp32_stream(d, relu, with_sc, use_mask, acc, ref.pattern)
            if integer:          # exact arithmetic: the fp32 run is the fp64 result, rounded stores included
                R.check_out('fp32', ref, R.bf(f['out']), True)
                R.check_apply('fp32', b, R.bf(f['dy']), R.bf(f['ds']), acc, True)
            else:
                R.check_out('fp32', ref, f['out'], False, frac=0.5)
                R.check_apply('fp32', b, f['dy'], f['ds'], acc, False, frac=0.5)
            n = R.n_sum(m, c)
            R.check_sums('fp32', 'bwd_reduce', f['sums'], b['sums'], b['m_sums'], b['x_sums'], n, integer, frac=0.5)
            R.check_sums('fp32', 'stats', f['stats'], ref.y2, ref.m_y2, torch.zeros(2, c), n, integer, frac=0.5)
            R.check_colsum('fp32', R.bf(f['out']), f['colsum'], m, c, integer, ref, frac=0.5)


@pytest.mark.parametrize('c', sorted(R.FINALIZE_ROWS))
def test_fp32_run_of_the_finalize_kernels_stays_inside_half_of_every_bound(c):
    for rows in R.FINALIZE_ROWS[c]:
        for integer in (True, False):
            p = R.finalize_rows(rows, c, integer)
            ref = R.FinalizeRef(p)
            assert bool((ref.var[2:] > 0).all()) and (integer or float(ref.var[1]) <= 1e-9)
            mu, rstd, scale, shift, rm, rv = R.fp32_finalize(p)
            ref.check('fp32', mu, rstd, scale, shift, rm, rv, frac=0.5)
            q = R.bwd_rows(rows, c, integer)
            for dzy, acc in ((0, 0), (0, 1), (1, 0)):
                coef, dg, db = R.fp32_bwd_finalize(q, dzy, acc)
                R.BwdFinalizeRef(q, dzy, acc).check('fp32', coef, dg, db, exact_sums=integer and not dzy, frac=0.5)
    p = R.finalize_rows(5, c, False)
    R.FinalizeRef(p, count=1).check('fp32', *R.fp32_finalize(p, count=1), frac=0.5)


@pytest.mark.parametrize('n,h,w,c', R.STEM_SHAPES)
def test_fp32_run_of_the_stem_stays_inside_half_of_every_bound(n, h, w, c):
    for integer in (True, False):
        d = R.stem_inputs(n, h, w, c, integer)
        ref = R.StemRef(d)
        b = ref.bwd(d, ref.tap)
        assert float(b['loose'].double().mean()) <= R.NEAR_SHARE
        pooled, tap, sums, dy = R.fp32_stem(d, ref)
        R.check_stem_fwd('fp32', d, ref, R.bf(pooled) if integer else pooled, tap.to(torch.uint8), ref.gather(d['y'], tap), integer, frac=0.5)
        if integer:
            assert 2 * float(b['m_sums'].max()) < 2 ** 24
            dy = R.bf(dy)
        R.check_stem_bwd('fp32', b, n * h * w, c, sums, dy, integer, frac=0.5)
        ps, pm = ref.pooled_sums(d, R.bf(ref.pooled), ref.ypool)
        if integer:       # every pooled element sends its gradient to one position: the pooled-domain sums are the position-domain ones
            assert torch.equal(ps, b['sums'])


def _autograd(y, gamma, beta, shortcut, relu, dout):
    yy = y.double().requires_grad_(True)
    z = F.batch_norm(yy, None, None, gamma.double(), beta.double(), True, 0.1, R.EPS)
    if shortcut is not None:
        z = z + shortcut.double()
    if relu:
        z = z.relu()
    z.backward(dout.double())
    return z.detach(), yy.grad


@pytest.mark.parametrize('relu,with_sc', [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_reference_agrees_with_batch_norm_autograd_in_fp64(relu, with_sc):
    m, c = 171, 24
    d = R.stream_inputs(m, c, False, seed=3)
    y = d['y'].double()
    gamma, beta = 1.0 + 0.3 * torch.randn(c, dtype=torch.float64), 0.3 * torch.randn(c, dtype=torch.float64)
    mu, var = y.mean(0), y.var(0, unbiased=False)
    rstd = (var + R.EPS) ** -0.5
    # the reference classes in fp64 parameters: statistics -> scale / shift -> out; sums -> coefficients -> dy
    st = torch.stack([y.sum(0), (y * y).sum(0)]).view(2, 1, c)
    fin = R.FinalizeRef(dict(stats=st, count=m, gamma=gamma, beta=beta, rm=torch.zeros(c), rv=torch.ones(c)))
    assert (fin.mean - mu).abs().max() < 1e-12 and (fin.rstd - rstd).abs().max() < 1e-10
    assert (fin.rv - (0.9 + float(torch.tensor(0.1, dtype=torch.float32)) * y.var(0, unbiased=True))).abs().max() < 1e-7
    d64 = dict(d, scale=fin.scale, shift=fin.shift, mean=fin.mean, rstd=fin.rstd)
    ref = R.StreamRef(d64, relu, with_sc)
    d64['coef'] = torch.zeros(3, c)
    b = ref.bwd(True, 0)
    bw = R.BwdFinalizeRef(dict(part=b['sums'].view(2, 1, c), m=m, gamma=gamma, mean=fin.mean, rstd=fin.rstd, pre=torch.zeros(2, c)))
    d64['coef'] = bw.coef
    b = ref.bwd(True, 0)
    out, dy = _autograd(d['y'], gamma, beta, d['shortcut'] if with_sc else None, relu, d['dout'])
    assert (ref.out - out).abs().max() < 1e-10
    assert (b['dy'] - dy).abs().max() < 1e-10
    # the chain reference is the same function
    if relu and with_sc:
        ch = R.ChainRef(d['y'], d['shortcut'], d['dout'], gamma.float(), beta.float())
        out32, dy32 = _autograd(d['y'], gamma.float(), beta.float(), d['shortcut'], 1, d['dout'])
        assert (ch.out - out32).abs().max() < 1e-10 and (ch.dy - dy32).abs().max() < 1e-10


def test_reference_agrees_with_the_fake_backend_within_the_bounds():
    m, c = 98, 72
    fake = FakeTok()
    d = R.stream_inputs(m, c, False, seed=1)
    for relu, with_sc, use_mask, acc in CONFIGS:
        ref = R.StreamRef(d, relu, with_sc)
        out, mask = torch.empty(m, c, dtype=BF), torch.empty(m, c // 8, dtype=torch.uint8)
        assert fake.tok_bn_act_fwd(P(d['y']), P(d['scale']), P(d['shift']), P(d['shortcut']) if with_sc else None, relu, P(out), P(mask),
                                   m, c, None) == 0
        R.check_out('fake', ref, out, False)
        R.check_mask(ref, out, unpack_bits(mask, m, c))
        b = ref.bwd(use_mask, acc)
        mk = ref.mask_bytes if use_mask else None
        part = torch.empty(2, 1, c)
        assert fake.tok_bn_bwd_reduce(P(d['dout']), P(d['y']), P(mk), P(d['scale']), P(d['shift']), P(d['mean']), P(d['rstd']), relu,
                                      m, c, P(part), None) == 0
        R.check_sums('fake', 'bwd_reduce', part.double().sum(1), b['sums'], b['m_sums'], b['x_sums'], m + 3, False)   # one row: m adds
        dy, ds = torch.empty(m, c, dtype=BF), d['ds0'].clone()
        if relu and not use_mask:
            ds = None
        assert fake.tok_bn_bwd_apply(P(d['dout']), P(d['y']), P(mk), P(d['scale']), P(d['shift']), P(d['coef']), relu, P(dy), P(ds), acc,
                                     m, c, None) == 0
        R.check_apply('fake', b, dy, ds, acc, False)
    for rows, c in ((65, 48), (17, 520)):
        p = R.finalize_rows(rows, c, False)
        mean, rstd, scale, shift = (torch.full((c,), 7.0) for _ in range(4))
        rm, rv, nbt = p['rm'].clone(), p['rv'].clone(), torch.tensor([4])
        assert fake.tok_bn_finalize(P(p['stats']), rows, p['count'], c, c - 3, P(p['gamma']), P(p['beta']), P(rm), P(rv), P(nbt), R.MOMENTUM,
                                    R.EPS, P(mean), P(rstd), P(scale), P(shift), None) == 0
        R.FinalizeRef(p, c_real=c - 3).check('fake', mean, rstd, scale, shift, rm[:c - 3], rv[:c - 3])
        assert int(nbt) == 5
        q = R.bwd_rows(rows, c, False)
        for dzy, acc in ((0, 0), (1, 1)):
            coef, dg, db = torch.full((3, c), 7.0), q['pre'][0].clone(), q['pre'][1].clone()
            assert fake.tok_bn_bwd_finalize(P(q['part']), rows, q['m'], c, c - 3, P(q['gamma']), P(q['mean']), P(q['rstd']), P(dg), P(db),
                                            P(coef), acc, dzy, None) == 0
            R.BwdFinalizeRef(q, dzy, acc, c_real=c - 3).check('fake', coef, dg[:c - 3], db[:c - 3])
    n, h, w, c = 2, 7, 9, 16
    d = R.stem_inputs(n, h, w, c, False)
    ref = R.StemRef(d)
    p_, q_ = d['dims'][4:]
    pooled, ypool = (torch.empty(n * p_ * q_, c, dtype=BF) for _ in range(2))
    arg = torch.empty(n * p_ * q_, c, dtype=torch.uint8)
    assert fake.tok_bn_relu_maxpool_fwd(P(d['y']), P(d['scale']), P(d['shift']), n, h, w, c, P(pooled), P(arg), P(ypool), None) == 0
    R.check_stem_fwd('fake', d, ref, pooled, arg, ypool, False)
    b = ref.bwd(d, ref.tap)
    tap8 = ref.tap.to(torch.uint8).contiguous()
    part, dy = torch.empty(2, 1, c), torch.empty(n * h * w, c, dtype=BF)
    assert fake.tok_bn_pool_bwd_reduce(P(d['dpool']), P(tap8), P(d['y']), P(d['scale']), P(d['shift']), P(d['mean']), P(d['rstd']),
                                       n, h, w, c, P(part), None) == 0
    assert fake.tok_bn_pool_bwd_apply(P(d['dpool']), P(tap8), P(d['y']), P(d['scale']), P(d['shift']), P(d['coef']), n, h, w, c, P(dy),
                                      None) == 0
    b1 = dict(b)
    R.check_sums('fake', 'pool_reduce', part.double().sum(1), b['sums'], b['m_sums'], b['x_sums'], n * h * w + 3, False)
    k = ~b1['loose']
    R.assert_bounded(dy[k], b['dy'][k], (R.B_DY * b['m_dy'] + 2 * b['e_dy'])[k], R.A_BF, 1.0, 'fake pool dy')


def test_near_zero_share_of_the_chosen_inputs():
    """the 0.1 % cap is a condition on the inputs and the fp64 reference alone: every shape, both patterns, and the stem"""
    for m, c in R.STREAM_SHAPES:
        d = R.stream_inputs(m, c, False)
        for with_sc in (0, 1):
            ref = R.StreamRef(d, 1, with_sc)
            assert float(ref.near.double().mean()) <= R.NEAR_SHARE and float(ref.near_rec.double().mean()) <= R.NEAR_SHARE
    for n, h, w, c in R.STEM_SHAPES:
        assert float(R.StemRef(R.stem_inputs(n, h, w, c, False)).near.double().mean()) <= R.NEAR_SHARE
    # the integer run has no such element at all: shift is a half-integer or an odd quarter
    d = R.stream_inputs(777, 48, True)
    assert float(R.StreamRef(d, 1, 1).z.abs().min()) >= 0.25 and float(R.StreamRef(d, 1, 0).z.abs().min()) >= 0.25


# ---- wrong variants do not pass ------------------------------------------------------------------------------------------------
def test_one_row_left_out_of_a_sum_fails():
    for m, c in ((777, 48), (1027, 2048)):
        for integer in (True, False):
            d = R.stream_inputs(m, c, integer)
            ref = R.StreamRef(d, 1, 1)
            b = ref.bwd(True, 0)
            d2 = dict(d, dout=d['dout'].clone(), y=d['y'].clone())
            f = R.fp32_stream(d, 1, 1, True, 0, ref.pattern)
            keep = torch.ones(m, 1)
            keep[m - 1] = 0
            xh = (d['y'].float() - d['mean']) * d['rstd']
            dz = d['dout'].float() * ref.pattern
            short = torch.stack([R.fp32_sum(dz * keep, m, c), R.fp32_sum(dz * xh * keep, m, c)])
            R.check_sums('x', 'bwd_reduce', f['sums'], b['sums'], b['m_sums'], b['x_sums'], R.n_sum(m, c), integer)
            with pytest.raises(AssertionError):
                R.check_sums('x', 'bwd_reduce', short, b['sums'], b['m_sums'], b['x_sums'], R.n_sum(m, c), integer)
            yf = d2['y'].float()
            with pytest.raises(AssertionError):
                R.check_sums('x', 'stats', torch.stack([R.fp32_sum(yf * keep, m, c), R.fp32_sum(yf * yf * keep, m, c)]), ref.y2, ref.m_y2,
                             torch.zeros(2, c), R.n_sum(m, c), integer)
    for rows, c in ((65, 48), (129, 520)):
        p = R.finalize_rows(rows, c, True)
        ref = R.FinalizeRef(p)
        short = dict(p, stats=p['stats'][:, :-1].contiguous())
        with pytest.raises(AssertionError):
            ref.check('x', *R.fp32_finalize(short))
        q = R.bwd_rows(rows, c, True)
        coef, dg, db = R.fp32_bwd_finalize(dict(q, part=q['part'][:, :-1]), 0, 0)
        with pytest.raises(AssertionError):
            R.BwdFinalizeRef(q).check('x', coef, dg, db, exact_sums=True)


def test_biased_running_variance_fails():
    p = R.finalize_rows(3, 48, False)          # count 96: unbias = 96 / 95
    ref = R.FinalizeRef(p)
    mu, rstd, scale, shift, rm, rv = R.fp32_finalize(p)
    ref.check('x', mu, rstd, scale, shift, rm, rv)
    S = p['stats'].double().sum(1)
    var = (S[1] / p['count'] - (S[0] / p['count']) ** 2).clamp_min(0).float()
    with pytest.raises(AssertionError):
        ref.check('x', mu, rstd, scale, shift, rm, 0.9 * p['rv'] + 0.1 * var)


def test_c2_and_c3_exchanged_fails():
    for integer in (True, False):
        d = R.stream_inputs(98, 72, integer)
        b = R.StreamRef(d, 1, 0).bwd(True, 0)
        c1, c2, c3 = d['coef']
        dz = b['dz'].float()
        with pytest.raises(AssertionError):
            R.check_apply('x', b, R.bf(c1 * dz + c3 * d['y'].float() + c2), None, 0, integer)
    q = R.bwd_rows(65, 48, False)
    coef, _, _ = R.fp32_bwd_finalize(q, 0, 0)
    with pytest.raises(AssertionError):
        R.BwdFinalizeRef(q).check('x', coef[[0, 2, 1]])


def test_shortcut_left_out_of_the_relu_pattern_fails():
    for integer in (True, False):
        d = R.stream_inputs(98, 72, integer)
        ref = R.StreamRef(d, 1, 1)
        b = ref.bwd(True, 0)
        f = R.fp32_stream(d, 1, 1, True, 0, ref.recomputed)        # the pattern of y * scale + shift alone
        with pytest.raises(AssertionError):
            R.check_apply('x', b, R.bf(f['dy']), None, 0, integer)
        with pytest.raises(AssertionError):
            R.check_sums('x', 'bwd_reduce', f['sums'], b['sums'], b['m_sums'], b['x_sums'], R.n_sum(98, 72), integer)
        with pytest.raises(AssertionError):
            R.check_mask(ref, R.bf(ref.out), ref.recomputed)


def test_fp32_one_pass_variance_fails_on_the_large_mean_channel():
    p = R.finalize_rows(64, 48, False)
    ref = R.FinalizeRef(p)
    n = p['count']
    S = p['stats'].double().sum(1).float()
    mu = S[0] / n
    rstd = torch.rsqrt(S[1] / n - mu * mu + R.EPS)
    good = R.fp32_finalize(p)
    R.assert_bounded(good[1][:1], ref.rstd[:1], ref.b_rstd[:1], 0.0, 1.0, 'rstd of the large-mean channel')
    with pytest.raises(AssertionError):
        R.assert_bounded(rstd[:1], ref.rstd[:1], ref.b_rstd[:1], 0.0, 1.0, 'rstd of the large-mean channel')
