"""The references and bounds of tests/metric_learning_ref.py, on a CPU:
  * every fp64 reference equals torch's own implementation in fp64, values and autograd gradients: F.normalize, the body of
    ArcFaceHead.__add_margin, torch.cdist with the ContrastiveLoss body, the regulariser's abs().sum / norm, nn.CrossEntropyLoss on the
    NT-Xent logits (-1e9 diagonal, labels (i + B) mod 2B), nn.TripletMarginLoss(p=2, eps, swap) — those few lines are restated here;
    the retrieval formulas equal oracle.retrieval_ref.meter_compute(per_query=True) on a classification and a representation set;
  * a plain fp32 run of every formula stays inside HALF of every bound on the inputs of every case of
    tests/test_metric_learning_contract_gpu.py (and, rounded once to bf16, inside the whole bound);
  * for every output tensor a deliberately wrong variant does NOT pass;
  * the three suspects of the contract module that can be decided on the host stand-in (tests/fake_backend.py): the refusals of
    tok_contrastive_bwd(same_tensor, n1 != n2) and of tok_relevance_matrix* past 2^31 - 1 elements, and the zero vector under
    normalize_vectors=True against the oracle."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fake_backend import FakeTok
from helpers import BF, F32
import metric_learning_ref as M
import oracle.retrieval_ref as O

F64 = torch.float64
P = lambda t: None if t is None else t.data_ptr()       # noqa: E731
TOL = dict(rtol=1e-11, atol=1e-12)


def half(what, mine32, out):
    """an fp32 run meets half of the fp32 part of the bound; rounded once to bf16 (where the kernel stores bf16) the whole bound"""
    w = M.check(None, what, mine32, out, frac=0.5, rounded=False)
    if bool((out.a > 0).any()):
        M.check(None, what + ' (bf16)', mine32.to(BF), out)
    return w


def rejected(what, wrong, out):
    with pytest.raises(AssertionError):
        M.check(None, what, wrong, out)


# ---- l2norm ------------------------------------------------------------------------------------------------------------------------
L2_CASES = [(r, c, f32) for r in M.ROWS for c, _ in M.COLS for f32 in (False, True)] + [(M.L2NORM_F32_EXTRA[0], M.L2NORM_F32_EXTRA[1], True)]


def test_l2norm_reference_is_f_normalize():
    for f32 in (False, True):
        x, dy, _ = M.make_l2norm(8, 65, f32, seed=1)
        xd = x.double().requires_grad_()
        y = F.normalize(xd, dim=1, eps=M.f32v(1e-12))
        y.backward(dy.double())
        inv, y64 = M.l2norm_fwd(x, 1e-12)
        torch.testing.assert_close(y64, y.detach(), **TOL)
        torch.testing.assert_close(M.l2norm_bwd(dy, y64, inv), xd.grad, **TOL)
    # the clamp branch: a row of norm 0.25 under eps = 1 is divided by 1
    x, _, _ = M.make_l2norm(8, 65, True, seed=1)
    torch.testing.assert_close(M.l2norm_fwd(x, 1.0)[1], F.normalize(x.double(), dim=1, eps=1.0), **TOL)
    assert abs(float(x[2].norm()) - 0.25) < 1e-3 and float(M.l2norm_fwd(x, 1.0)[0][2]) == 1.0


@pytest.mark.parametrize('rows,c,f32', L2_CASES)
def test_l2norm_fp32_run_stays_inside_half_of_every_bound(rows, c, f32):
    x, dy, prior = M.make_l2norm(rows, c, f32, seed=rows + c)
    for eps in (1e-12, 1.0):
        ref = M.l2norm_fwd_ref(x, eps)
        inv32, y32 = M.l2norm_fwd(x, eps, F32)
        half('inv_norm', inv32, ref['inv_norm'])
        half('y', y32, ref['y'])
        ys = y32 if f32 else y32.to(BF)
        for pr in (None, prior):
            half('dx', M.l2norm_bwd(dy, ys, inv32, pr, F32), M.l2norm_bwd_ref(dy, ys, inv32, pr)['dx'])


def test_l2norm_wrong_variants_are_rejected():
    x, dy, prior = M.make_l2norm(8, 65, False, seed=2)
    ref = M.l2norm_fwd_ref(x, 1.0)
    xf = x.float()
    nrm = xf.pow(2).sum(1).sqrt()
    rejected('inv_norm without the clamp', 1 / nrm.clamp_min(1e-30), ref['inv_norm'])
    rejected('y without the clamp', xf / nrm.clamp_min(1e-30)[:, None], ref['y'])
    inv32, y32 = M.l2norm_fwd(x, 1e-12, F32)
    rejected('dx without the projection', dy.float() * inv32[:, None], M.l2norm_bwd_ref(dy, y32.to(BF), inv32)['dx'])
    rejected('dx that overwrites under accumulate', M.l2norm_bwd(dy, y32.to(BF), inv32, None, F32), M.l2norm_bwd_ref(dy, y32.to(BF), inv32, prior)['dx'])


# ---- ArcFace ---------------------------------------------------------------------------------------------------------------------------
def _add_margin(cosine, target, p):
    """the body of ArcFaceHead.__add_margin (restated), on float64 cosines"""
    sine = torch.sqrt((1.0 - torch.pow(cosine, 2)).clamp(0, 1))
    phi = (cosine * p.cos_m - sine * p.sin_m).type(cosine.dtype)
    phi = torch.where(cosine > 0, phi, cosine) if p.easy else torch.where(cosine > p.th, phi, cosine - p.mm)
    one_hot = torch.zeros_like(cosine)
    one_hot.scatter_(1, target.view(-1, 1).long(), 1)
    return torch.where(one_hot == 1, phi, cosine) * p.scale


ARC_P = [M.ArcP(0.5, 30.0, 0), M.ArcP(0.5, 30.0, 1), M.ArcP(0.35, 64.0, 0, th=-0.9375)]


@pytest.mark.parametrize('p', ARC_P, ids=['hard', 'easy', 'hard-th-bf16'])
def test_arcface_reference_is_add_margin(p):
    cs, t, dout = M.make_arcface(37, 65, p, seed=3)
    ok = (t >= 0) & (t < 65)
    assert int((~ok).sum()) == 2
    cd = cs.double()[ok].requires_grad_()
    out = _add_margin(cd, t[ok], p)
    out.backward(dout.double()[ok])
    mine, _ = M.arcface_fwd(cs, t, p, round_phi=False)
    torch.testing.assert_close(mine[ok], out.detach(), **TOL)
    assert torch.equal(mine[~ok], cs.double()[~ok] * p.scale), 'a target outside [0, classes) changes no column'
    g, _ = M.arcface_bwd(cs, t, dout, p)
    # autograd is not finite at cos = +-1 (rows 0, 1) and the fp32 clamp decides cos = 2^-14 (row 6): the documented rule there
    plain = torch.ones(37, dtype=torch.bool)
    plain[[0, 1, 6]] = False
    mine_g, auto = g[ok & plain], cd.grad[plain[ok]]
    fin = torch.isfinite(auto)                    # (autograd of the unselected branch of torch.where is 0 * inf where |cos| == 1)
    assert bool((cs.double()[ok & plain][~fin].abs() == 1).all()) and bool(torch.isfinite(mine_g).all())
    torch.testing.assert_close(mine_g[fin], auto[fin], **TOL)
    for r in (0, 1, 6):
        use = bool(M._arc_use(cs, p)[r, t[r]])
        assert float(g[r, t[r]]) == float(dout[r, t[r]]) * p.scale * (p.cos_m if use else 1.0)
    if p.th == -0.9375:
        assert float(cs[3, t[3]]) == p.th and float(cs[4, t[4]]) < p.th < float(cs[5, t[5]]), 'exactly th and its bf16 neighbours'
        use = M._arc_use(cs, p)
        assert [bool(use[r, t[r]]) for r in (3, 4, 5)] == [False, False, True]


@pytest.mark.parametrize('rows,classes,ld,grid', M.ARC_CASES)
def test_arcface_fp32_run_stays_inside_half_of_every_bound(rows, classes, ld, grid):
    for p in (ARC_P if rows < 100 else ARC_P[:1]):
        cs, t, dout = M.make_arcface(rows, classes, p, seed=rows)
        ref, n_tie = M.arcface_fwd_ref(cs, t, p)
        assert n_tie <= 2, 'the rounding-tie slack is for a handful of elements'
        half('out', M.arcface_fwd(cs, t, p, F32)[0], ref['out'])
        half('dcos', M.arcface_bwd(cs, t, dout, p, F32)[0], M.arcface_bwd_ref(cs, t, dout, p)['dcos'])


def test_arcface_wrong_variants_are_rejected():
    p = ARC_P[0]
    cs, t, dout = M.make_arcface(131, 65, p, seed=4)
    ref, _ = M.arcface_fwd_ref(cs, t, p)
    rejected('phi not rounded', M.arcface_fwd(cs, t, p, F32, round_phi=False)[0].to(BF), ref['out'])
    g32, dsn = M.arcface_bwd(cs, t, dout, p, F32)
    oh = M._onehot(t, 131, 65) & M._arc_use(cs, p)
    wrong = torch.where(oh, dout.float() * p.scale * (p.cos_m - dsn * p.sin_m), g32)
    rejected('sine term with the wrong sign', wrong, M.arcface_bwd_ref(cs, t, dout, p)['dcos'])


# ---- relevance ---------------------------------------------------------------------------------------------------------------------
def test_relevance_references_are_exact_and_wrong_variants_differ():
    la, lb = M.make_labels(7, 130, seed=5)
    R = M.relevance(la, lb)
    assert not torch.equal(R, (la.int()[:, None] == lb.int()[None, :]).float()), 'labels that differ only above bit 32'
    for classes in M.ML_CLASSES:
        ya, yb = M.make_multilabel(7, 130, classes, seed=classes)
        R64, R32 = M.relevance_ml(ya, yb), M.relevance_ml(ya, yb, F32)
        assert torch.equal(R64, R32), 'dyadic labels: fp32 and fp64 agree bit for bit'
        assert torch.equal(R64, (ya.double() @ yb.double().t() > 0).float())
        assert not torch.equal(R64, (ya @ yb.t() >= 0).float())
        assert float(R64[0].sum()) == 0 and float(R64[6, 129]) == 0, 'a zero row and a negative product are not relevant'


# ---- contrastive -------------------------------------------------------------------------------------------------------------------
def _contrastive_torch(e1, e2, R, mu):
    S = torch.cdist(e1, e2, p=2, compute_mode='donot_use_mm_for_euclid_dist')
    L = (1. - R) * F.relu(mu - S).pow(2) + R * S.pow(2)
    return S, L.sum(1)


@pytest.mark.parametrize('same', [False, True])
def test_contrastive_reference_is_cdist_with_the_loss_body(same):
    e1, e2, R = M.make_contrastive(8, 8 if same else 5, 20, seed=6, same=same)
    a = e1.double().requires_grad_()
    b = a if same else e2.double().requires_grad_()
    S, rl = _contrastive_torch(a, b, R.double(), M.f32v(1.0))
    (rl.mean() * 0.7).backward()
    S64, rl64 = M.contrastive_fwd(e1, e2, R, 1.0)
    torch.testing.assert_close(S64, S.detach(), **TOL)
    torch.testing.assert_close(rl64, rl.detach(), **TOL)
    g1, g2 = M.contrastive_bwd(e1, e2, R, S64, 1.0, 0.7)
    if same:
        torch.testing.assert_close(g1 + g2, a.grad, **TOL)
    else:
        torch.testing.assert_close(g1, a.grad, **TOL)
        torch.testing.assert_close(g2, b.grad, **TOL)
        assert float(S64[0, 0]) == 0 and float(S64[1, 1]) == 0 and float(R[0, 0]) == 0 and float(R[1, 1]) == 1
        assert float(S64[2, 2]) == 1.0, 'a pair exactly at the margin'


@pytest.mark.parametrize('n1,n2,d,ld,same', M.CONTRASTIVE_CASES)
def test_contrastive_fp32_run_stays_inside_half_of_every_bound(n1, n2, d, ld, same):
    for r_mode in ('mixed', '0', '1'):
        e1, e2, R = M.make_contrastive(n1, n2, d, seed=n1 + n2, same=same, r_mode=r_mode)
        ref = M.contrastive_fwd_ref(e1, e2, R, 1.0)
        S32, rl32 = M.contrastive_fwd(e1, e2, R, 1.0, F32)
        half('S', S32, ref['S'])
        half('row_loss', rl32, ref['row_loss'])
        M.check_mean(None, 'loss', rl32.double().mean().float(), rl32)
        g1, g2 = M.contrastive_bwd(e1, e2, R, S32, 1.0, 0.7, F32)
        bref = M.contrastive_bwd_ref(e1, e2, R, S32, 1.0, 0.7, same)
        if same:
            half('de1', g1 + g2, bref['de1'])
            M.check(None, 'de1 stored between the launches', (g1.to(BF).float() + g2).to(BF), bref['de1'])
        else:
            half('de1', g1, bref['de1'])
            half('de2', g2, bref['de2'])


def test_contrastive_wrong_variants_are_rejected():
    e1, e2, R = M.make_contrastive(33, 65, 129, seed=7)
    ref = M.contrastive_fwd_ref(e1, e2, R, 1.0)
    S32, rl32 = M.contrastive_fwd(e1, e2, R, 1.0, F32)
    rejected('S without the root', S32 * S32, ref['S'])
    rejected('row_loss with R and 1 - R exchanged', M.contrastive_fwd(e1, e2, 1 - R, 1.0, F32)[1], ref['row_loss'])
    with pytest.raises(AssertionError):
        M.check_mean(None, 'loss as a sum', rl32.sum(), rl32)
    bref = M.contrastive_bwd_ref(e1, e2, R, S32, 1.0, 0.7)
    g1, g2 = M.contrastive_bwd(e1, e2, R, S32, 1.0, 0.7, F32, scale_n1=False)
    rejected('de1 without 1 / n1', g1, bref['de1'])
    g1, g2 = M.contrastive_bwd(e1, e2, R, S32, 1.0, 0.7, F32)
    rejected('de2 with the sign of de1', -g2, bref['de2'])
    e1, e2, R = M.make_contrastive(8, 8, 65, seed=8, same=True)
    S32 = M.contrastive_fwd(e1, e2, R, 1.0, F32)[0]
    g1, g2 = M.contrastive_bwd(e1, e2, R, S32, 1.0, 0.7, F32)
    rejected('same tensor, second operand dropped', g1, M.contrastive_bwd_ref(e1, e2, R, S32, 1.0, 0.7, True)['de1'])


# ---- embedding regulariser -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [1, 2])
def test_embed_reg_reference_is_the_regulariser(mode):
    e = M.make_embed(8, 65, seed=9)
    x = e.double().requires_grad_()
    rr = x.abs().sum(1) if mode == 1 else torch.norm(x, p=None, dim=1)
    (rr.mean() * 0.7 * 8 * 0.001).backward()            # gscale coeff per row (the caller folds 1 / n into coeff)
    rr64 = M.embed_reg_fwd(e, mode)
    torch.testing.assert_close(rr64, rr.detach(), **TOL)
    torch.testing.assert_close(M.embed_reg_bwd(e, rr64, M.f32v(0.7), M.f32v(0.001), mode), x.grad, rtol=1e-7, atol=1e-12)
    assert bool((x.grad[0] == 0).all()) and float(x.grad[7, 0]) == 0, 'the zero row and the -0.0 element get gradient 0'


EMBED_CASES = [(n, c) for n in (1, 5, 8, 131, 256, 257) for c, _ in M.COLS]


@pytest.mark.parametrize('n,d', EMBED_CASES)
def test_embed_reg_fp32_run_stays_inside_half_of_every_bound(n, d):
    e = M.make_embed(n, d, seed=n + d)
    for mode in (1, 2):
        rr32 = M.embed_reg_fwd(e, mode, F32)
        half('row_reg', rr32, M.embed_reg_fwd_ref(e, mode)['row_reg'])
        M.check_mean(None, 'out', rr32.double().mean().float(), rr32)
        half('de', M.embed_reg_bwd(e, rr32, 0.7, 0.001, mode, F32), M.embed_reg_bwd_ref(e, rr32, 0.7, 0.001, mode)['de'])


def test_embed_reg_wrong_variants_are_rejected():
    e = M.make_embed(8, 65, seed=9)
    rr32 = M.embed_reg_fwd(e, 2, F32)
    rejected('row_reg of the other mode', M.embed_reg_fwd(e, 1, F32), M.embed_reg_fwd_ref(e, 2)['row_reg'])
    with pytest.raises(AssertionError):
        M.check_mean(None, 'out as a sum', rr32.sum(), rr32)
    rejected('de without the norm', e.float() * M.f32v(0.7) * M.f32v(0.001), M.embed_reg_bwd_ref(e, rr32, 0.7, 0.001, 2)['de'])


# ---- NT-Xent -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm,t', [(1.0, 0.5), (4.0, 0.1)])
def test_ntxent_reference_is_cross_entropy_of_the_logits(norm, t):
    e = M.make_ntxent(6, 20, seed=10, norm=norm)
    x = e.double().requires_grad_()
    B = 3
    sim = torch.matmul(x, x.transpose(1, 0)) / M.f32v(t)
    sim = sim.masked_fill(torch.eye(2 * B, dtype=torch.bool), -1e9)
    labels = torch.cat([torch.arange(B, 2 * B), torch.arange(B)])
    rows = torch.nn.CrossEntropyLoss(reduction='none')(sim, labels)
    (torch.nn.CrossEntropyLoss()(sim, labels) * 0.7).backward()
    lse, rl = M.ntxent_fwd(e, t)
    torch.testing.assert_close(rl, rows.detach(), rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(lse, torch.logsumexp(sim.detach(), 1), **TOL)
    torch.testing.assert_close(M.ntxent_bwd(e, lse, t, 0.7), x.grad, rtol=1e-9, atol=1e-11)


NTX_CASES = [(n, d, norm, t) for n in M.NTX_N for d, _ in M.NTX_D for norm, t in ((1.0, 0.5), (4.0, 0.1))]


@pytest.mark.parametrize('n,d,norm,t', NTX_CASES)
def test_ntxent_fp32_run_stays_inside_half_of_every_bound(n, d, norm, t):
    e = M.make_ntxent(n, d, seed=n + d, norm=norm)
    ref = M.ntxent_fwd_ref(e, t)
    if norm > 1 and n >= 64:
        z, _ = M.ntxent_logits(e, t)
        off = z.masked_fill(torch.eye(n, dtype=torch.bool), math.nan)
        assert float(np.nanmax(off.numpy()) - np.nanmin(off.numpy())) > 100, 'norms near 4, T = 0.1: the logits span more than 100'
    lse32, rl32 = M.ntxent_fwd(e, t, F32)
    half('lse', lse32, ref['lse'])
    half('row_loss', rl32, ref['row_loss'])
    half('demb', M.ntxent_bwd(e, lse32, t, 0.7, F32), M.ntxent_bwd_ref(e, lse32, t, 0.7)['demb'])


def test_ntxent_wrong_variants_are_rejected():
    e = M.make_ntxent(64, 64, seed=11)
    t = 0.5
    ref = M.ntxent_fwd_ref(e, t)
    z, lab = M.ntxent_logits(e, t, F32)
    zu = (e.float() @ e.float().t()) / t
    rejected('lse with the diagonal in the sum', torch.logsumexp(zu, 1), ref['lse'])
    lse32, rl32 = M.ntxent_fwd(e, t, F32)
    rejected('row_loss with label (i + B - 1) mod n', lse32 - z.gather(1, ((lab - 1) % 64)[:, None])[:, 0], ref['row_loss'])
    with pytest.raises(AssertionError):
        M.check_mean(None, 'loss as a sum', rl32.sum(), rl32)
    bref = M.ntxent_bwd_ref(e, lse32, t, 0.7)['demb']
    rejected('demb with label (i + B - 1) mod n', M.ntxent_bwd(e, lse32, t, 0.7, F32, label_shift=-1), bref)
    rejected('demb without 1 / T', M.ntxent_bwd(e, lse32, t, 0.7, F32, use_inv_t=False), bref)


# ---- triplet -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('swap', [0, 1])
@pytest.mark.parametrize('eps', [1e-6, 0.0])
def test_triplet_reference_is_triplet_margin_loss(swap, eps):
    a, p, n = M.make_triplet(8, 65, seed=12)
    A, Pp, N = (v.double().requires_grad_() for v in (a, p, n))
    e = M.f32v(eps)
    fn = torch.nn.TripletMarginLoss(margin=M.f32v(0.3), p=2, eps=e, swap=bool(swap), reduction='none')
    rows = fn(A, Pp, N)
    (rows.mean() * 0.7).backward()
    dist, rl = M.triplet_fwd(a, p, n, 0.3, eps, swap)
    torch.testing.assert_close(rl, rows.detach(), **TOL)
    got = M.triplet_bwd(a, p, n, dist, 0.3, eps, swap, 0.7)
    keep = torch.ones(8, dtype=torch.bool)
    if eps == 0.0:
        keep[0] = False                 # anchor == positive: ||0||'s autograd is not finite; the kernel's rule is a zero direction
        assert float(dist[0, 0]) == 0 and bool((got[2][0] == -got[0][0]).all()) and bool(torch.isfinite(got[0]).all())
    if swap:
        # anchor == positive makes d_pn == d_an exactly: torch.min's autograd splits a tie half and half, the kernel (dpn < dan is
        # false) keeps d_an, which is a subgradient too: the row equals the rule without swap
        keep[0] = False
        assert float(dist[0, 1]) == float(dist[0, 2])
        for mine, plain in zip(got, M.triplet_bwd(a, p, n, dist, 0.3, eps, 0, 0.7)):
            assert torch.equal(mine[0], plain[0])
    for mine, leaf in zip(got, (A, Pp, N)):
        torch.testing.assert_close(mine[keep], leaf.grad[keep], **TOL)
    sw, active = M.triplet_branches(dist, 0.3, swap)
    assert not bool(active[1]) and bool((got[0][1] == 0).all()), 'a row with zero loss has gradient exactly 0'
    if swap:
        assert bool(sw[2]) and not bool(sw[3]) and bool(active[2]) and bool(active[3]), 'the swap takes effect in row 2 only'


TRIP_CASES = [(r, c) for r in M.ROWS for c, _ in M.COLS]


@pytest.mark.parametrize('rows,d', TRIP_CASES)
def test_triplet_fp32_run_stays_inside_half_of_every_bound(rows, d):
    a, p, n = M.make_triplet(rows, d, seed=rows + d)
    for swap in (0, 1):
        for eps in (1e-6, 0.0):
            ref = M.triplet_fwd_ref(a, p, n, 0.3, eps, swap)
            d32, rl32 = M.triplet_fwd(a, p, n, 0.3, eps, swap, F32)
            half('dist', d32, ref['dist'])
            half('row_loss', rl32, ref['row_loss'])
            bref = M.triplet_bwd_ref(a, p, n, d32, 0.3, eps, swap, 0.7)
            for what, g in zip(('d_anchor', 'd_positive', 'd_negative'), M.triplet_bwd(a, p, n, d32, 0.3, eps, swap, 0.7, F32)):
                half(what, g, bref[what])


def test_triplet_wrong_variants_are_rejected():
    a, p, n = M.make_triplet(8, 65, seed=12)
    ref = M.triplet_fwd_ref(a, p, n, 0.3, 1e-6, 1)
    d32, rl32 = M.triplet_fwd(a, p, n, 0.3, 1e-6, 1, F32)
    rejected('dist without eps', M.triplet_fwd(a, p, n, 0.3, 0.0, 1, F32)[0], ref['dist'])
    rejected('row_loss with the swap ignored', M.triplet_fwd(a, p, n, 0.3, 1e-6, 0, F32)[1], ref['row_loss'])
    with pytest.raises(AssertionError):
        M.check_mean(None, 'loss as a sum', rl32.sum(), rl32)
    bref = M.triplet_bwd_ref(a, p, n, d32, 0.3, 1e-6, 1, 0.7)
    wrong = M.triplet_bwd(a, p, n, d32, 0.3, 1e-6, 1, 0.7, F32, honour_swap=False)
    for what, g in zip(('d_anchor', 'd_positive', 'd_negative'), wrong):
        rejected(what + ' with the swap ignored', g, bref[what])
    for what, g in zip(('d_anchor', 'd_positive'), M.triplet_bwd(a, p, n, d32, 0.3, 1e-6, 1, 0.7, F32, use_eps=False)):
        rejected(what + ' without eps', g, bref[what])              # row 0: anchor == positive, the direction is eps / ||eps||


# ---- similarity matrix and top-k ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nq,ng,d', M.SIM_CASES)
def test_sim_matrix_and_topk(nq, ng, d):
    q, g = M.make_sim(nq, ng, d, seed=nq + d)
    for metric in (0, 1):
        ref = M.sim_matrix_ref(q, g, metric)['out']
        want = q.double() @ g.double().t() if metric == 0 else -torch.cdist(q.double(), g.double(), compute_mode='donot_use_mm_for_euclid_dist').pow(2)
        torch.testing.assert_close(ref.ref, want, rtol=1e-10, atol=1e-12)
        s32 = M.sim_matrix(q, g, metric, F32)
        half('out', s32, ref)
        rejected('out with the other sign', -s32 + (0 if d > 1 or metric else 1e-3), ref)
        # on tie-free rows the ranking is the oracle's flat search and torch.topk
        k = min(ng, 5)
        vals, idx = M.topk_rows(s32, k)
        ov, oi = O.flat_search(g.numpy(), q.numpy(), k, 'IP' if metric == 0 else 'L2')
        if nq * ng > 1:
            assert np.array_equal(idx.numpy(), oi)
        tv, ti = torch.topk(s32, k, dim=1)
        assert torch.equal(vals, tv) and torch.equal(idx, ti)


def test_topk_reference_ties_padding_and_nan():
    s = M.make_topk(8, 70, seed=13)
    for k in (1, 70, 73):
        vals, idx = M.topk_rows(s, k)
        assert idx[0].tolist() == list(range(min(k, 70))) + [-1] * max(k - 70, 0), 'all equal: index order'
        assert idx[1].tolist() == list(range(min(k, 70))) + [-1] * max(k - 70, 0) and bool((vals[1] == -math.inf).all()), '-inf ranks'
        assert int(idx[2, 0]) == 35 and float(vals[2, 0]) == math.inf
        assert bool((idx[3] == -1).all()) and bool((vals[3] == -math.inf).all()), 'NaN never ranks'
        assert idx[4].tolist()[:min(k, 70)] == list(range(min(k, 70))), '-0.0 == +0.0: index order'
        live = int((~torch.isnan(s[5])).sum())
        assert bool((idx[5, :min(k, live)] % 3 != 0).all()) and bool((idx[5, live:] == -1).all())
        if k > 1:
            wv, wi = M.topk_rows(s, k, reverse_ties=True)
            assert torch.equal(wv, vals) and not torch.equal(wi, idx), 'reversed tie order: same values, other indices'


# ---- retrieval: n_rel and the five metrics against the oracle ------------------------------------------------------------------------------
def _oracle_problem(kind_data, k, seed):
    """what IndexBasedMeter.compute feeds tok_retrieval_nrel / _eval, built from the oracle's own bookkeeping"""
    rng = np.random.RandomState(seed)
    n, d = 40, 8
    vec = rng.randn(n, d).astype(np.float32)
    kk = k + 1
    if kind_data == 'classification':
        labels = rng.randint(0, 4, n)
        _, gallery, q_rows, q_as_rel = O.prepare_classification(labels)
        q_cols, scores = None, None
        args = dict(group_labels=labels)
    else:
        labels = np.zeros(n, np.int64)
        query_idxs = -np.ones(n, np.int64)
        query_idxs[:6] = np.arange(6)
        scores = rng.choice([0.0, 0.0, 0.0, 1.0, 2.0, 3.0], size=(n, 6)).astype(np.float32)
        scores[:6] = 0
        scores[2, 3] = 2.0                                        # one query that is relevant to another: it stays in the gallery
        _, gallery, q_cols, q_rows, q_as_rel = O.prepare_representation(query_idxs, scores)
        args = dict(group_labels=labels, query_idxs=query_idxs, scores=scores)
    _, local = O.flat_search(vec[gallery], vec[q_rows], kk, 'IP')
    t = lambda a, dt=torch.int64: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt)   # noqa: E731
    prob = dict(idx=t(local), drop_first=t(q_as_rel.astype(np.uint8), torch.uint8), gallery=t(gallery), ng=len(gallery),
                labels=t(labels) if kind_data == 'classification' else None, scores=t(scores, F32), q_row=t(q_rows), q_col=t(q_cols), ideal=None)
    prob['n_rel'] = M.nrel(prob['labels'], prob['scores'], prob['q_row'], prob['q_col'])
    if scores is not None:
        gains = torch.where(prob['scores'] >= 1, prob['scores'], torch.zeros(()))[:, prob['q_col']].t()
        prob['ideal'] = torch.sort(gains, 1, descending=True).values[:, :k].contiguous()
    return vec, args, prob


@pytest.mark.parametrize('kind_data', ['classification', 'representation'])
@pytest.mark.parametrize('k', [2, 7])
def test_retrieval_reference_is_the_oracle_per_query(kind_data, k):
    vec, args, prob = _oracle_problem(kind_data, k, seed=14)
    for kind, name in enumerate(M.KINDS):
        _, per_q = O.meter_compute(name, vec, kind_data, k=k, per_query=True, **args)
        mine = M.retrieval_eval(kind, prob['idx'], prob['drop_first'], prob['gallery'], prob['ng'], prob['labels'], prob['scores'],
                                prob['q_row'], prob['q_col'], prob['n_rel'], prob['ideal'])
        want = torch.tensor([per_q[int(r)] for r in prob['q_row']], dtype=F64)
        torch.testing.assert_close(mine, want, rtol=1e-13, atol=0)
        assert float(want.max()) > 0


@pytest.mark.parametrize('kind_data', ['classification', 'representation'])
def test_retrieval_wrong_variants_are_rejected(kind_data):
    pr = M.make_retrieval(kind_data, 50, 257, 6, seed=15, use_gallery=True)
    a = (pr['idx'], pr['drop_first'], pr['gallery'], pr['ng'], pr['labels'], pr['scores'], pr['q_row'], pr['q_col'], pr['n_rel'], pr['ideal'])
    assert int((pr['n_rel'] == 0).sum()) > 0 and int((pr['n_rel'] > 5).sum()) > 0 and int(((pr['n_rel'] > 0) & (pr['n_rel'] < 5)).sum()) > 0
    if kind_data == 'classification':
        assert not torch.equal(M.nrel(pr['labels'], None, pr['q_row'], None, keep_self=True), pr['n_rel'])
    else:
        assert not torch.equal((pr['scores'][:, pr['q_col']] > 0).sum(0).int(), pr['n_rel']), 'a score just below 1 is not relevant'
    for kind in range(5):
        ref = M.eval_out(M.retrieval_eval(kind, *a))
        M.check(None, 'out', ref.ref.float(), ref)
        rejected('drop_first inverted', M.retrieval_eval(kind, *a, invert_drop=True).float(), ref)
    ref = M.eval_out(M.retrieval_eval(4, *a))
    rejected('ndcg with k in place of min(k, n_rel)', torch.nan_to_num(M.retrieval_eval(4, *a[:9], None, ndcg_k_only=True)).float(),
             M.eval_out(M.retrieval_eval(4, *a[:9], None)))


# ---- the suspects, on the host stand-in ------------------------------------------------------------------------------------------------
def test_contrastive_bwd_same_tensor_needs_n1_equal_n2():
    """tok_contrastive_bwd(same_tensor = 1) accumulates the n2 rows of the second operand onto de1, which holds n1 rows: refused
    unless n1 == n2 (include/tok.h).  The stand-in refuses like the library."""
    lib = FakeTok()
    e1, e2, R = M.make_contrastive(5, 3, 20, seed=16)
    S = M.contrastive_fwd(e1, e2, R, 1.0, F32)[0].contiguous()
    de1 = torch.full((5, 20), 9.0, dtype=BF)
    assert lib.tok_contrastive_bwd(P(e1), P(e2), P(R), P(S), None, 5, 3, 20, 20, 1.0, P(de1), None, 1, None) == -1
    assert bool((de1 == 9.0).all())
    assert lib.tok_contrastive_bwd(P(e1), P(e1), P(R), P(S), None, 3, 3, 20, 20, 1.0, P(de1), None, 1, None) == 0


def test_relevance_matrix_refuses_more_than_int_max_elements():
    lib = FakeTok()
    la = torch.zeros(4, dtype=torch.int64)
    R = torch.full((16,), 9.0)
    ya = torch.zeros(4, 2)
    assert lib.tok_relevance_matrix(P(la), P(la), 65536, 32768, P(R), None) == -1
    assert lib.tok_relevance_matrix_multilabel(P(ya), P(ya), 46341, 46341, 2, P(R), None) == -1
    assert bool((R == 9.0).all())
    assert lib.tok_relevance_matrix(P(la), P(la), 4, 4, P(R), None) == 0 and bool((R == 1.0).all())


def test_zero_vector_under_normalize_vectors_on_the_host_stand_in(fake_backend):
    """the meter-level pin of tests/test_metric_learning_contract_gpu.py::test_zero_vector_under_normalize_vectors, on the stand-in:
    the zero vector becomes NaN as in the reference (0 / 0), is retrieved by nobody and retrieves k + 1 times -1; the expected
    values are oracle.retrieval_ref.meter_compute(normalize_vectors=True), whose flat_search drops NaN as faiss's result heap does"""
    res = M.run_zero_vector_meter('cpu')
    for name, (got, want, zero_query) in res.items():
        assert abs(got - want) <= 1e-6 * max(abs(want), 1e-30), (name, got, want)
    assert res['precision'][2] == 1.0 and res['recall'][2] == 3 / 5


def test_oracle_flat_search_never_returns_a_nan_score():
    """oracle.retrieval_ref.flat_search: a gallery row of NaN is retrieved by nobody, a query of NaN retrieves k labels of -1, for
    both metrics; without NaN it is the stable argsort it was (lower index on ties, -1 past the gallery size)"""
    g = np.array([[1, 0], [np.nan, np.nan], [1, 0], [0, 1]], np.float32)
    q = np.array([[1, 0], [np.nan, np.nan]], np.float32)
    for metric, pad in (('IP', -np.inf), ('L2', np.inf)):
        val, idx = O.flat_search(g, q, 5, metric)
        assert idx.tolist() == [[0, 2, 3, -1, -1], [-1] * 5], (metric, idx)
        assert not np.isnan(val).any() and (val[1] == pad).all() and (val[0, 3:] == pad).all()
