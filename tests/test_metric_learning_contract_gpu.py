"""The metric-learning entries of csrc/metric.hip (tok_l2norm_*, tok_arcface_margin_*, tok_relevance_matrix*, tok_contrastive_*,
tok_embed_reg_*, tok_ntxent_*, tok_triplet_*) and the retrieval entries of csrc/retrieval.hip (tok_sim_matrix, tok_topk_rows,
tok_retrieval_nrel, tok_retrieval_eval) element by element against fp64 of the same inputs; references, bounds, input makers and
the case lists are in tests/metric_learning_ref.py (tests/test_metric_learning_ref.py: every reference is torch's own operation in
fp64, an fp32 run stays inside half of every bound, wrong variants are rejected).  No element is excluded from any comparison.

Every input sits behind NaN pads and NaN guards, every output in a sentinel-filled guarded buffer; after each call the guards are
intact, every owned element is written and finite, and the pad columns hold what include/tok.h says (zero, or untouched).  Every
backward runs twice and must be bit-identical (the kernels use no atomics).  Every case names the launch class it is meant to hit and
asserts it against a restatement of the launcher's rule, so that a threshold change moves a test instead of silently moving coverage:
  one wave per row (l2norm, contrastive, embed_reg_fwd, NT-Xent, triplet, top-k, n_rel): blocks of four waves — a lone wave, a ragged
      last block, full blocks, many blocks; the lanes stride c: below, at and above 64 columns, NT-Xent's 16 register slots (d <= 1024)
  grid_for (ArcFace, embed_reg_bwd): below one block / several blocks / past the 4096-block cap (a second grid-stride trip)
  mean_kernel (every loss[0], the regulariser's out[0]): n below, at and above its 256 threads
  sim_kernel: 64 x 64 tiles, K in steps of 16 — partial tiles in both directions, d below / at / above a K step
  eval_kernel: one thread per query, nq below and above one 256-thread block
Three suspected defects are decided in test_refusals (same_tensor with n1 != n2, na * nb past 2^31 - 1: both were launched
before, both are refused now) and test_zero_vector_under_normalize_vectors (correct as it was: see its docstring).
The worst |err| / bound of every tensor of every kernel family goes to profiles/metric_learning_contract_parity_distances.json;
profiles/metric_learning_contract_mutation_check.txt lists the hand-made kernel defects this module was run against.

On an MI355X the module (182 tests) runs in 4.9 s; the slowest case is the first one, test_l2norm[1-...-1-8-...-bf16], 0.48 s (it pays
the first launch), then test_triplet[1-...-1-8-...], 0.13 s; every other case is below 0.07 s (ArcFace 129 x 8131: 0.05 s)."""
import math

import numpy as np
import pytest
import torch

from helpers import BF, ERR_INVALID, F32, GuardedSpan, Mat, cdiv, last_error
import metric_learning_ref as M
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
I64, I32, U8 = torch.int64, torch.int32, torch.uint8
P = lambda t: None if t is None else t.data_ptr()       # noqa: E731
TAG = 'metric_learning_contract/'


@pytest.fixture(autouse=True, scope='module')
def _parity_record():
    """one line per kernel family and tensor: the worst |err| / bound over every case and variant of the family"""
    yield
    M.flush_record()


def wave_class(rows):
    """one wavefront per row, four to a 256-thread block: grid = cdiv(rows, 4)"""
    return f'{cdiv(rows, 4)} block{"s" if rows > 4 else ""}, {"ragged" if rows % 4 else "full"}'


WAVES = [(1, '1 block, ragged'), (5, '2 blocks, ragged'), (8, '2 blocks, full'), (131, '33 blocks, ragged')]


def lane_class(c):
    """the 64 lanes of a wave stride the columns"""
    return 'below 64' if c < 64 else 'exactly 64' if c == 64 else f'{cdiv(c, 64)} trips'


LANES = [(1, 8, 'below 64'), (20, 24, 'below 64'), (63, 64, 'below 64'), (64, 64, 'exactly 64'), (65, 72, '2 trips'), (129, 129, '3 trips'),
         (1000, 1000, '16 trips')]
assert tuple((c, ld) for c, ld, _ in LANES) == M.COLS and tuple(r for r, _ in WAVES) == M.ROWS


def mean_class(n):
    """mean_kernel: one block of 256 threads strides the n row values"""
    return 'below 256' if n < 256 else 'exactly 256' if n == 256 else 'second trip'


def grid_class(total):
    b = cdiv(total, 256)
    assert M.grid_for(total) == min(max(b, 1), 4096)
    return 'below one block' if total < 256 else 'blocks' if b <= 4096 else 'second trip'


def mat_in(t, ld=None, off=0):
    """an input [rows][cols] of pitch ld: NaN in the pads, in front and in both guards"""
    t = t if t.dim() == 2 else t.reshape(1, -1)
    return Mat(t.shape[0], t.shape[1], ld, dtype=t.dtype, init=t.cuda(), nan=True, off=off)


def vec_out(n, dtype=F32):
    return Mat(1, n, dtype=dtype)


def scalar_out():
    return GuardedSpan(1, F32, 64)


def scalar_done(lo, what):
    lo.check(what)
    assert not lo.untouched() and math.isfinite(float(lo.view[0])), what


def _gs(v):
    return None if v is None else torch.tensor([v], dtype=F32, device='cuda')


def bits(m):
    """every element of the buffer behind a Mat / GuardedSpan, as integers (bit-identity, pads and guards included)"""
    b = m.span.buf if isinstance(m, Mat) else m.buf
    return b.view({2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[b.element_size()]).clone()


def ok(rc, what):
    _C.check(rc, what)
    torch.cuda.synchronize()


# ---- l2norm ------------------------------------------------------------------------------------------------------------------------
def _l2norm(rows, c, ld, f32, off=0):
    lib, st = _C.lib(), stream_ptr()
    tag = TAG + ('l2norm_f32' if f32 else 'l2norm_bf16')
    dt = F32 if f32 else BF
    x, dy, prior = M.make_l2norm(rows, c, f32, seed=rows + c)
    xg = mat_in(x, ld, off)
    for eps in (1e-12, 1.0):
        ref = M.l2norm_fwd_ref(x, eps)
        yg, ig = Mat(rows, c, ld, dtype=dt, off=off), vec_out(rows)
        ok(lib.tok_l2norm_fwd(xg.ptr, yg.ptr, ig.ptr, rows, c, ld, int(f32), eps, st), 'l2norm_fwd')
        xg.done('x', finite=False)
        yg.done('y', zero_pads=True)
        ig.done('inv_norm')
        M.check(tag, 'inv_norm', ig.view[0], ref['inv_norm'])
        M.check(tag, 'y', yg.view, ref['y'])
        if rows > 1:
            assert bool((yg.view[0] == 0).all()) and float(ig.view[0, 0]) == float(np.float32(1) / np.float32(eps)), 'a zero row: y = 0, inv = 1 / eps'
        if rows > 2 and eps == 1.0:
            assert float(ig.view[0, 2]) == 1.0, 'a row of norm 0.25 under eps = 1 takes the clamp branch'
        y, inv = yg.value(), ig.value()[0]
        y_in, i_in, dy_in = mat_in(y, ld), mat_in(inv), mat_in(dy, ld, off)
        for pr in (None, prior):
            bref = M.l2norm_bwd_ref(dy, y, inv, pr)['dx']
            runs = []
            for _ in range(2):
                dg = Mat(rows, c, ld, dtype=dt, init=None if pr is None else pr.cuda())
                ok(lib.tok_l2norm_bwd(dy_in.ptr, y_in.ptr, i_in.ptr, dg.ptr, int(pr is not None), rows, c, ld, int(f32), st), 'l2norm_bwd')
                # fresh: the pad columns are written 0; accumulate: they keep what they held (re-stored as read)
                dg.done('dx', zero_pads=pr is None)
                runs.append(bits(dg))
            assert torch.equal(runs[0], runs[1]), 'l2norm_bwd is not deterministic'
            M.check(tag, 'dx' if pr is None else 'dx accumulated', dg.view, bref)
        for m_, what in ((y_in, 'y'), (i_in, 'inv_norm'), (dy_in, 'dy')):
            m_.done(what, finite=False)


@pytest.mark.parametrize('f32', [False, True], ids=['bf16', 'f32'])
@pytest.mark.parametrize('c,ld,lanes', LANES)
@pytest.mark.parametrize('rows,waves', WAVES)
def test_l2norm(rows, waves, c, ld, lanes, f32):
    assert wave_class(rows) == waves and lane_class(c) == lanes
    _l2norm(rows, c, ld, f32)


def test_l2norm_f32_long_row_and_offset_operands():
    """(3, 2049): 33 trips of the lanes with one element in the last; operands 8 and 3 elements past a 16-byte boundary.  There is no
    in-place case: include/tok.h rules x == y out."""
    r, c, ld = M.L2NORM_F32_EXTRA
    assert lane_class(c) == '33 trips'
    _l2norm(r, c, ld, True)
    _l2norm(5, 65, 72, False, off=8)
    _l2norm(5, 65, 72, True, off=3)


# ---- ArcFace ---------------------------------------------------------------------------------------------------------------------------
ARC_P = [M.ArcP(0.5, 30.0, 0), M.ArcP(0.5, 30.0, 1), M.ArcP(0.35, 64.0, 0, th=-0.9375)]


@pytest.mark.parametrize('rows,classes,ld,grid', M.ARC_CASES)
def test_arcface(rows, classes, ld, grid):
    """target columns at cos = 1, -1, 0, th (a bf16 value in the third parameter set: exactly th) and its bf16 neighbours, 2^-14;
    targets -1 and == classes; hard and easy margin"""
    lib, st = _C.lib(), stream_ptr()
    assert grid_class(rows * ld) == grid
    ties = 0
    for p in (ARC_P if rows < 100 else ARC_P[:1]):
        cs, t, dout = M.make_arcface(rows, classes, p, seed=rows)
        cg, tg, dg_in = mat_in(cs, ld), mat_in(t), mat_in(dout, ld)
        ref, n_tie = M.arcface_fwd_ref(cs, t, p)
        ties += n_tie
        og = Mat(rows, classes, ld)
        ok(lib.tok_arcface_margin_fwd(cg.ptr, tg.ptr, rows, classes, ld, *p.args(), og.ptr, st), 'arcface_fwd')
        og.done('out', zero_pads=True)
        M.check(TAG + 'arcface', 'out', og.view, ref['out'])
        if rows > 8:
            for r in (7, 8):
                assert torch.equal(og.value()[r].float(), (cs[r].float() * p.scale).to(BF).float()), 'a target outside [0, classes) changes no column'
        runs = []
        for _ in range(2):
            dc = Mat(rows, classes, ld)
            ok(lib.tok_arcface_margin_bwd(cg.ptr, tg.ptr, dg_in.ptr, rows, classes, ld, *p.args(), dc.ptr, st), 'arcface_bwd')
            dc.done('dcos', zero_pads=True)
            runs.append(bits(dc))
        assert torch.equal(runs[0], runs[1]), 'arcface_bwd is not deterministic'
        M.check(TAG + 'arcface', 'dcos', dc.view, M.arcface_bwd_ref(cs, t, dout, p)['dcos'])
        for m_, what in ((cg, 'cosine'), (tg, 'target'), (dg_in, 'dout')):
            m_.done(what, finite=False)
    print(f'arcface {rows}x{classes}: {ties} target elements took the rounding-tie slack')
    assert ties <= 2, 'the slack is for a handful of elements: at most 2 in total over the parameter sets of one case'


# ---- relevance ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('na,nb', M.REL_CASES)
def test_relevance(na, nb):
    """exact; labels that differ only above bit 32; (256, 256) is 256 full blocks, (7, 130) ends in a ragged one, (1, 1) is one thread"""
    lib, st = _C.lib(), stream_ptr()
    la, lb = M.make_labels(na, nb, seed=na + nb)
    if na * nb > 1:
        la[0], lb[0], lb[nb - 1] = 3, 3 + 2 ** 32, 3
    lag, lbg, rg = mat_in(la), mat_in(lb), Mat(na, nb, dtype=F32)
    ok(lib.tok_relevance_matrix(lag.ptr, lbg.ptr, na, nb, rg.ptr, st), 'relevance')
    rg.done('R')
    assert torch.equal(rg.value(), M.relevance(la, lb)), 'R'
    if na * nb > 1:
        assert float(rg.view[0, 0]) == 0 and float(rg.view[0, nb - 1]) == 1
    for classes in M.ML_CLASSES:
        ya, yb = M.make_multilabel(na, nb, classes, seed=classes + na)
        yag, ybg, mg = mat_in(ya), mat_in(yb), Mat(na, nb, dtype=F32)
        ok(lib.tok_relevance_matrix_multilabel(yag.ptr, ybg.ptr, na, nb, classes, mg.ptr, st), 'relevance_ml')
        mg.done('R multilabel')
        for m_ in (yag, ybg):
            m_.done('labels', finite=False)
        assert torch.equal(mg.value(), M.relevance_ml(ya, yb)), f'R multilabel, {classes} classes'
    for m_ in (lag, lbg):
        m_.done('labels', finite=False)


# ---- contrastive -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n1,n2,d,ld,same', M.CONTRASTIVE_CASES)
def test_contrastive(n1, n2, d, ld, same):
    """duplicate rows with R = 0 and R = 1 (S == 0), a pair exactly at the margin, R mixed / all zero / all one; (300, 7): mean_kernel's
    second trip; (8, 8): one tensor, de1 stored as bf16 between the two launches"""
    lib, st = _C.lib(), stream_ptr()
    assert mean_class(n1) == ('second trip' if n1 == 300 else 'below 256')
    tag = TAG + ('contrastive_same' if same else 'contrastive')
    for r_mode in ('mixed', '0', '1'):
        e1, e2, R = M.make_contrastive(n1, n2, d, seed=n1 + n2, same=same, r_mode=r_mode)
        g1 = mat_in(e1, ld)
        g2 = g1 if same else mat_in(e2, ld)
        rg = mat_in(R)
        sg, rl, lo = Mat(n1, n2, dtype=F32), vec_out(n1), scalar_out()
        ok(lib.tok_contrastive_fwd(g1.ptr, g2.ptr, rg.ptr, n1, n2, d, ld, 1.0, sg.ptr, rl.ptr, lo.ptr, st), 'contrastive_fwd')
        sg.done('S')
        rl.done('row_loss')
        scalar_done(lo, 'loss')
        ref = M.contrastive_fwd_ref(e1, e2, R, 1.0)
        M.check(tag, 'S', sg.view, ref['S'])
        M.check(tag, 'row_loss', rl.view[0], ref['row_loss'])
        M.check_mean(tag, 'loss[0] vs its own rows', lo.view[:1], rl.view[0])
        if not same and min(n1, n2) > 2 and r_mode == 'mixed':
            assert float(sg.view[0, 0]) == 0 and float(sg.view[1, 1]) == 0 and float(sg.view[2, 2]) == 1.0
        S = sg.value()
        s_in = mat_in(S)
        for gs in (0.7, None):
            bref = M.contrastive_bwd_ref(e1, e2, R, S, 1.0, 1.0 if gs is None else gs, same)
            runs = []
            for _ in range(2):
                d1, d2 = Mat(n1, d, ld), None if same else Mat(n2, d, ld)
                ok(lib.tok_contrastive_bwd(g1.ptr, g2.ptr, rg.ptr, s_in.ptr, P(_gs(gs)), n1, n2, d, ld, 1.0, d1.ptr, None if same else d2.ptr,
                                           int(same), st), 'contrastive_bwd')
                d1.done('de1', zero_pads=True)
                runs.append(bits(d1))
                if not same:
                    d2.done('de2', zero_pads=True)
                    runs.append(bits(d2))
            assert all(torch.equal(a, b) for a, b in zip(runs[:len(runs) // 2], runs[len(runs) // 2:])), 'contrastive_bwd is not deterministic'
            M.check(tag, 'de1', d1.view, bref['de1'])
            if not same:
                M.check(tag, 'de2', d2.view, bref['de2'])
        for m_, what in ((g1, 'e1'), (g2, 'e2'), (rg, 'R'), (s_in, 'S')):
            m_.done(what, finite=False)


# ---- embedding regulariser -----------------------------------------------------------------------------------------------------------
def _embed(n, d, ld, grid=None):
    lib, st = _C.lib(), stream_ptr()
    e = M.make_embed(n, d, seed=n + d)
    eg = mat_in(e, ld)
    for mode in (1, 2):
        tag = TAG + f'embed_reg_l{mode}'
        rg, lo = vec_out(n), scalar_out()
        ok(lib.tok_embed_reg_fwd(eg.ptr, n, d, ld, mode, rg.ptr, lo.ptr, st), 'embed_reg_fwd')
        rg.done('row_reg')
        scalar_done(lo, 'out')
        M.check(tag, 'row_reg', rg.view[0], M.embed_reg_fwd_ref(e, mode)['row_reg'])
        M.check_mean(tag, 'out[0] vs its own rows', lo.view[:1], rg.view[0])
        rr = rg.value()[0]
        r_in = mat_in(rr)
        runs = []
        for _ in range(2):
            dg = Mat(n, d, ld)
            ok(lib.tok_embed_reg_bwd(eg.ptr, r_in.ptr, P(_gs(0.7)), 0.001, n, d, ld, mode, dg.ptr, st), 'embed_reg_bwd')
            dg.done('de', zero_pads=True)
            runs.append(bits(dg))
        assert torch.equal(runs[0], runs[1]), 'embed_reg_bwd is not deterministic'
        M.check(tag, 'de', dg.view, M.embed_reg_bwd_ref(e, rr, 0.7, 0.001, mode)['de'])
        if n > 1:
            assert bool((dg.view[0] == 0).all()), 'a zero row has gradient 0'
        assert float(dg.view[n - 1, 0]) == 0, 'an element that is -0.0 has gradient 0'
        r_in.done('row_reg', finite=False)
    eg.done('e', finite=False)


@pytest.mark.parametrize('c,ld,lanes', LANES)
@pytest.mark.parametrize('rows,waves', WAVES)
def test_embed_reg(rows, waves, c, ld, lanes):
    assert wave_class(rows) == waves and lane_class(c) == lanes
    _embed(rows, c, ld)


@pytest.mark.parametrize('n,mean', [(256, 'exactly 256'), (257, 'second trip')])
def test_embed_reg_mean_kernel_classes(n, mean):
    assert mean_class(n) == mean and mean_class(1) == 'below 256'         # (n = 1 is in test_embed_reg)
    _embed(n, 20, 24)


def test_embed_reg_bwd_past_the_grid_cap():
    """129 x 8136 elements: 4100 blocks of 256, capped at 4096 — the last 968 elements are a second grid-stride trip"""
    rows, d, ld, grid = M.ARC_CASES[2]
    assert grid_class(rows * ld) == 'second trip' == grid
    _embed(rows, d, ld)


# ---- NT-Xent -----------------------------------------------------------------------------------------------------------------------
def ntx_slots(d):
    """ntxent_bwd_kernel keeps 16 columns per lane in registers: d <= 1024; the last slot holds columns 960 .. 1023"""
    assert d <= 16 * 64
    return cdiv(d, 64)


@pytest.mark.parametrize('d,ld,slots', [(20, 24, 1), (64, 64, 1), (961, 968, 16), (1023, 1024, 16), (1024, 1024, 16)])
@pytest.mark.parametrize('n,waves', [(2, '1 block, ragged'), (6, '2 blocks, ragged'), (64, '16 blocks, full'), (258, '65 blocks, ragged')])
def test_ntxent(n, waves, d, ld, slots):
    """unit-norm embeddings at T = 0.5 and norms near 4 at T = 0.1 (logits spanning more than 100: the online-softmax rescale and the
    flush-to-zero tail); rows 0 and 1 identical; gscale present and NULL"""
    lib, st = _C.lib(), stream_ptr()
    assert wave_class(n) == waves and ntx_slots(d) == slots and (n, (d, ld)) in [(a, b) for a in M.NTX_N for b in M.NTX_D]
    assert mean_class(n) == ('second trip' if n == 258 else 'below 256')
    for norm, t in ((1.0, 0.5), (4.0, 0.1)):
        tag = TAG + ('ntxent_unit' if norm == 1.0 else 'ntxent_large_norm')
        e = M.make_ntxent(n, d, seed=n + d, norm=norm)
        eg = mat_in(e, ld)
        lg, rl, lo = vec_out(n), vec_out(n), scalar_out()
        ok(lib.tok_ntxent_fwd(eg.ptr, n, d, ld, t, lg.ptr, rl.ptr, lo.ptr, st), 'ntxent_fwd')
        lg.done('lse')
        rl.done('row_loss')
        scalar_done(lo, 'loss')
        ref = M.ntxent_fwd_ref(e, t)
        M.check(tag, 'lse', lg.view[0], ref['lse'])
        M.check(tag, 'row_loss', rl.view[0], ref['row_loss'])
        M.check_mean(tag, 'loss[0] vs its own rows', lo.view[:1], rl.view[0])
        lse = lg.value()[0]
        l_in = mat_in(lse)
        for gs in (0.7, None):
            runs = []
            for _ in range(2):
                dg = Mat(n, d, ld)
                ok(lib.tok_ntxent_bwd(eg.ptr, l_in.ptr, P(_gs(gs)), n, d, ld, t, dg.ptr, st), 'ntxent_bwd')
                dg.done('demb', zero_pads=True)
                runs.append(bits(dg))
            assert torch.equal(runs[0], runs[1]), 'ntxent_bwd is not deterministic'
            M.check(tag, 'demb', dg.view, M.ntxent_bwd_ref(e, lse, t, 1.0 if gs is None else gs)['demb'])
        eg.done('emb', finite=False)
        l_in.done('lse', finite=False)


# ---- triplet -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c,ld,lanes', LANES)
@pytest.mark.parametrize('rows,waves', WAVES)
def test_triplet(rows, waves, c, ld, lanes):
    """both swap values (row 2: the swap takes effect, row 3: it does not), a row with zero loss (gradients exactly 0), anchor == positive
    with eps = 1e-6 and eps = 0 (the dap == 0 branch)"""
    lib, st = _C.lib(), stream_ptr()
    assert wave_class(rows) == waves and lane_class(c) == lanes
    a, p, n = M.make_triplet(rows, c, seed=rows + c)
    ag, pg, ng = mat_in(a, ld), mat_in(p, ld), mat_in(n, ld)
    for swap in (0, 1):
        tag = TAG + f'triplet_swap{swap}'
        for eps in (1e-6, 0.0):
            dg, rl, lo = Mat(rows, 3, dtype=F32), vec_out(rows), scalar_out()
            ok(lib.tok_triplet_fwd(ag.ptr, pg.ptr, ng.ptr, rows, c, ld, 0.3, eps, swap, dg.ptr, rl.ptr, lo.ptr, st), 'triplet_fwd')
            dg.done('dist')
            rl.done('row_loss')
            scalar_done(lo, 'loss')
            ref = M.triplet_fwd_ref(a, p, n, 0.3, eps, swap)
            M.check(tag, 'dist', dg.view, ref['dist'])
            M.check(tag, 'row_loss', rl.view[0], ref['row_loss'])
            M.check_mean(tag, 'loss[0] vs its own rows', lo.view[:1], rl.view[0])
            dist = dg.value()
            if eps == 0.0:
                assert float(dist[0, 0]) == 0, 'anchor == positive, eps = 0: d_ap is exactly 0'
            sw, active = M.triplet_branches(dist, 0.3, swap)
            if rows > 3 and c >= 20:
                assert not bool(active[1]) and bool(active[0]) and (not swap or (bool(sw[2]) and not bool(sw[3])))
            d_in = mat_in(dist)
            for gs in (0.7, None):
                bref = M.triplet_bwd_ref(a, p, n, dist, 0.3, eps, swap, 1.0 if gs is None else gs)
                runs = []
                for _ in range(2):
                    outs = [Mat(rows, c, ld) for _ in range(3)]
                    ok(lib.tok_triplet_bwd(ag.ptr, pg.ptr, ng.ptr, d_in.ptr, P(_gs(gs)), rows, c, ld, 0.3, eps, swap, outs[0].ptr, outs[1].ptr,
                                           outs[2].ptr, st), 'triplet_bwd')
                    for o, what in zip(outs, ('d_anchor', 'd_positive', 'd_negative')):
                        o.done(what, zero_pads=True)
                    runs.append([bits(o) for o in outs])
                assert all(torch.equal(x, y) for x, y in zip(*runs)), 'triplet_bwd is not deterministic'
                for o, what in zip(outs, ('d_anchor', 'd_positive', 'd_negative')):
                    M.check(tag, what, o.view, bref[what])
                    assert bool((o.view[~active.cuda()] == 0).all()), 'a row with zero loss has gradient exactly 0'
            d_in.done('dist', finite=False)
    for m_, what in ((ag, 'anchor'), (pg, 'positive'), (ng, 'negative')):
        m_.done(what, finite=False)


# ---- similarity matrix and top-k ---------------------------------------------------------------------------------------------------
def sim_class(nq, ng, d):
    """64 x 64 output tiles, K in steps of 16"""
    return f'{cdiv(ng, 64)}x{cdiv(nq, 64)} tiles{"" if nq % 64 or ng % 64 else ", full"}, {cdiv(d, 16)} K steps{"" if d % 16 else ", full"}'


SIM_IDS = ['1x1 tiles, 1 K steps', '2x1 tiles, 1 K steps', '1x1 tiles, full, 1 K steps, full', '3x2 tiles, 2 K steps', '2x3 tiles, 13 K steps']


@pytest.mark.parametrize('case,cls', list(zip(M.SIM_CASES, SIM_IDS)))
def test_sim_matrix_and_topk_of_it(case, cls):
    """both metrics; ldq, ldg and ldo all above their minimum, with NaN pads; then the k best of the pitched matrix (ld > cols, NaN in the
    pads), k in {1, cols, cols + 3}, against the exact ranking of the kernel's own matrix"""
    lib, st = _C.lib(), stream_ptr()
    nq, ng, d = case
    assert sim_class(nq, ng, d) == cls
    q, g = M.make_sim(nq, ng, d, seed=nq + d)
    qg, gg = mat_in(q, d + 3), mat_in(g, d + 5, off=3)
    for metric in (0, 1):
        og = Mat(nq, ng, ng + 7, dtype=F32)
        ok(lib.tok_sim_matrix(qg.ptr, gg.ptr, nq, ng, d, d + 3, d + 5, metric, og.ptr, ng + 7, st), 'sim_matrix')
        og.done('out')
        M.check(TAG + ('sim_ip' if metric == 0 else 'sim_l2'), 'out', og.view, M.sim_matrix_ref(q, g, metric)['out'])
        s = og.value()
        s_in = mat_in(s, ng + 7)
        for k in (1, ng, ng + 3):
            vg, ig = Mat(nq, k, dtype=F32), Mat(nq, k, dtype=I64)
            ok(lib.tok_topk_rows(s_in.ptr, nq, ng, ng + 7, k, vg.ptr, ig.ptr, st), 'topk_rows')
            vg.done('vals', finite=False)
            ig.done('idx')
            vals, idx = M.topk_rows(s, k)
            assert torch.equal(vg.value(), vals) and torch.equal(ig.value(), idx), f'top-{k} of {ng}'
        s_in.done('s', finite=False)
    qg.done('q', finite=False)
    gg.done('g', finite=False)


@pytest.mark.parametrize('rows,waves', WAVES)
@pytest.mark.parametrize('cols,ld', [(1, 4), (63, 64 + 1), (70, 77), (129, 140)])
def test_topk_rows_ties_infinities_and_nan(rows, waves, cols, ld):
    """exact.  A row of all equal values, of all -inf, with a +inf, of all NaN, of -0.0 against +0.0, with NaN scattered among values;
    many ties everywhere; k in {1, cols, cols + 3}"""
    lib, st = _C.lib(), stream_ptr()
    assert wave_class(rows) == waves
    s = M.make_topk(rows, cols, seed=rows + cols)
    sg = mat_in(s, ld)
    for k in (1, cols, cols + 3):
        vg, ig = Mat(rows, k, dtype=F32), Mat(rows, k, dtype=I64)
        ok(lib.tok_topk_rows(sg.ptr, rows, cols, ld, k, vg.ptr, ig.ptr, st), 'topk_rows')
        vg.done('vals', finite=False)
        ig.done('idx')
        vals, idx = M.topk_rows(s, k)
        assert torch.equal(ig.value(), idx), f'idx, top-{k} of {cols}'
        assert torch.equal(vg.value().view(I32), vals.view(I32)) or torch.equal(vg.value(), vals), f'vals, top-{k} of {cols}'
        assert not bool(torch.isnan(vg.value()).any()), 'NaN never ranks'
    sg.done('s', finite=False)


# ---- retrieval: n_rel and the per-query metrics ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_gallery', [False, True], ids=['identity', 'gallery'])
@pytest.mark.parametrize('kind_data', ['classification', 'representation'])
@pytest.mark.parametrize('nq,blocks', [(1, 1), (5, 1), (257, 2)])
def test_retrieval_nrel_and_eval(nq, blocks, kind_data, use_gallery):
    """all five metrics per query; an index row with -1; drop_first mixed within the call; queries with n_rel == 0, n_rel < k and
    n_rel > k; graded scores with a value just below 1.0 (not relevant); nDCG with and without `ideal`; n_rel: one wave per query"""
    lib, st = _C.lib(), stream_ptr()
    assert cdiv(nq, 256) == blocks and nq in M.EVAL_NQ
    n, kk = 50, 6
    pr = M.make_retrieval(kind_data, n, nq, kk, seed=nq + 15, use_gallery=use_gallery)
    cls = kind_data == 'classification'
    lab = mat_in(pr['labels']) if cls else None
    sc = None if cls else mat_in(pr['scores'])
    n_cols = 0 if cls else pr['scores'].shape[1]
    qr, qc = mat_in(pr['q_row']), None if cls else mat_in(pr['q_col'])
    gal = mat_in(pr['gallery']) if use_gallery else None
    ix, dr = mat_in(pr['idx']), mat_in(pr['drop_first'])
    mp = lambda m_: None if m_ is None else m_.ptr      # noqa: E731
    ng_ = vec_out(nq, I32)
    ok(lib.tok_retrieval_nrel(mp(lab), mp(sc), n, n_cols, qr.ptr, mp(qc), nq, ng_.ptr, st), 'retrieval_nrel')
    ng_.done('n_rel')
    assert torch.equal(ng_.value()[0], pr['n_rel']), 'n_rel'
    if nq > 2:
        assert int(pr['n_rel'][0]) == 0 and 0 < int(pr['n_rel'][1 if cls else 2]) < kk - 1 and int(pr['n_rel'].max()) > kk - 1
    nr = mat_in(pr['n_rel'])
    ideals = [None] if cls else [pr['ideal'], None]
    for kind in range(5):
        for ideal in (ideals if kind == 4 else ideals[:1]):
            idl = None if ideal is None else mat_in(ideal)
            og = vec_out(nq)
            ok(lib.tok_retrieval_eval(kind, ix.ptr, kk, dr.ptr, mp(gal), pr['ng'], mp(lab), mp(sc), n_cols, qr.ptr, mp(qc), nr.ptr, mp(idl), nq,
                                      og.ptr, st), 'retrieval_eval')
            og.done('out')
            want = M.retrieval_eval(kind, pr['idx'], pr['drop_first'], pr['gallery'], pr['ng'], pr['labels'], pr['scores'], pr['q_row'],
                                    pr['q_col'], pr['n_rel'], ideal)
            M.check(TAG + 'retrieval_eval', M.KINDS[kind], og.view[0], M.eval_out(want))
            if idl is not None:
                idl.done('ideal', finite=False)
    for m_ in (lab, sc, qr, qc, gal, ix, dr, nr):
        if m_ is not None:
            m_.done('input', finite=False)


# ---- the zero vector under normalize_vectors ---------------------------------------------------------------------------------------------
def test_zero_vector_under_normalize_vectors():
    """Suspect 3, decided: the call is right as it is.  tok_l2norm_fwd with eps = 0 makes the zero vector NaN exactly as the
    reference's division does, and tok_topk_rows never ranks a NaN: the meter equals oracle.retrieval_ref.meter_compute(
    normalize_vectors=True) for all five metrics, and the oracle's flat_search states why (faiss's result heap admits a score only
    where a comparison with it holds, which is never for a NaN; a query without results gets labels -1, read as the last gallery
    row).  The oracle's search used to argsort the NaN row (gallery rows 0 .. k for the zero-vector query) and was corrected with
    this test: faiss itself is not available to the suite, the heap rule is the evidence.  A positive eps would keep the zero
    vector at inner product 0 with everything: it would then rank above every negative cosine, which the reference never does.
    The same case runs on the host stand-in in tests/test_metric_learning_ref.py."""
    res = M.run_zero_vector_meter('cuda')
    for name, (got, want, zero_query) in res.items():
        assert abs(got - want) <= 1e-6 * max(abs(want), 1e-30), (name, got, want)
    # the zero-vector query retrieves k times the last gallery row, which carries its label: every position is a hit
    assert res['precision'][2] == 1.0 and res['recall'][2] == 3 / 5


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(rc, what):
    assert rc == ERR_INVALID, (what, rc, last_error())


def _null_each(fn, args, required, what):
    """every required pointer replaced by NULL in turn"""
    for i in required:
        a = list(args)
        assert a[i] is not None
        a[i] = None
        _refused(fn(*a), f'{what}: argument {i} NULL')


def test_refusals():
    """valid call, refused calls, the same valid call again (bit-identical): a refused call returns TOK_ERR_INVALID before any launch and
    writes nothing.  Includes the two refusals this module added: tok_contrastive_bwd(same_tensor = 1) with n1 != n2 (the second launch
    wrote n2 rows into the n1 rows of de1) and tok_relevance_matrix* with na * nb > 2^31 - 1 (the int index and the grid wrapped;
    asked with small valid buffers: nothing is launched at that size)."""
    lib, st = _C.lib(), stream_ptr()
    rows, c, ld = 5, 20, 24
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device='cuda')        # noqa: E731
    x, tgt, lab = z(rows, ld), z(rows, dt=I64), z(rows, dt=I64)
    xf, R, S, vec3 = z(rows, ld, dt=F32), z(rows, rows, dt=F32), z(rows, rows, dt=F32), z(rows, 3, dt=F32)
    v = z(rows, dt=F32)
    gs = _gs(1.0)
    u8, i32 = z(rows, dt=U8), z(rows, dt=I32)
    ix = z(rows, 3, dt=I64)
    outs = dict(bf=[Mat(rows, ld, ld) for _ in range(3)], f=[Mat(rows, rows, dtype=F32) for _ in range(3)], lo=scalar_out(), i64=Mat(rows, 3, dtype=I64),
                i32=Mat(1, rows, dtype=I32), f6=Mat(rows + 1, ld + 8, dtype=F32))
    b0, b1, b2 = (m.ptr for m in outs['bf'])
    f0, f1, f2 = (m.ptr for m in outs['f'])
    lo, o64, o32 = outs['lo'].ptr, outs['i64'].ptr, outs['i32'].ptr
    X, T_, L, XF, RR, SS, V3, V, G, U, N32, IX = (P(t) for t in (x, tgt, lab, xf, R, S, vec3, v, gs, u8, i32, ix))
    arc = M.ArcP().args()

    def valid():
        """one valid call of EVERY entry (contrastive_bwd in both forms) into fresh outputs; returns the bits of all of them"""
        bfm = lambda: Mat(rows, c, ld)                                  # noqa: E731
        sq, v1 = (lambda: Mat(rows, rows, dtype=F32)), (lambda: vec_out(rows))      # noqa: E731
        ms = []

        def new(*makers):
            made = [mk() for mk in makers]
            ms.extend(made)
            return [m.ptr for m in made]
        y, inv = new(bfm, v1)
        ok(lib.tok_l2norm_fwd(X, y, inv, rows, c, ld, 0, 1e-12, st), 'l2norm_fwd')
        dx, = new(bfm)
        ok(lib.tok_l2norm_bwd(X, X, V, dx, 0, rows, c, ld, 0, st), 'l2norm_bwd')
        o, dc = new(bfm, bfm)
        ok(lib.tok_arcface_margin_fwd(X, T_, rows, c, ld, *arc, o, st), 'arcface_fwd')
        ok(lib.tok_arcface_margin_bwd(X, T_, X, rows, c, ld, *arc, dc, st), 'arcface_bwd')
        r1, r2 = new(sq, sq)
        ok(lib.tok_relevance_matrix(L, L, rows, rows, r1, st), 'relevance')
        ok(lib.tok_relevance_matrix_multilabel(XF, XF, rows, rows, c, r2, st), 'relevance_ml')
        s_, rl, l0 = new(sq, v1, scalar_out)
        ok(lib.tok_contrastive_fwd(X, X, RR, rows, rows, c, ld, 1.0, s_, rl, l0, st), 'contrastive_fwd')
        d1, d2, d3 = new(bfm, bfm, bfm)
        ok(lib.tok_contrastive_bwd(X, X, RR, SS, G, rows, rows, c, ld, 1.0, d1, d2, 0, st), 'contrastive_bwd')
        ok(lib.tok_contrastive_bwd(X, X, RR, SS, G, rows, rows, c, ld, 1.0, d3, None, 1, st), 'contrastive_bwd (one tensor)')
        rr, l1, de = new(v1, scalar_out, bfm)
        ok(lib.tok_embed_reg_fwd(X, rows, c, ld, 1, rr, l1, st), 'embed_reg_fwd')
        ok(lib.tok_embed_reg_bwd(X, V, G, 0.1, rows, c, ld, 1, de, st), 'embed_reg_bwd')
        ls, rn, l2, dn = new(v1, v1, scalar_out, bfm)
        ok(lib.tok_ntxent_fwd(X, 4, c, ld, 0.5, ls, rn, l2, st), 'ntxent_fwd')
        ok(lib.tok_ntxent_bwd(X, V, G, 4, c, ld, 0.5, dn, st), 'ntxent_bwd')
        ds, rt, l3, ta, tp, tn = new(lambda: Mat(rows, 3, dtype=F32), v1, scalar_out, bfm, bfm, bfm)
        ok(lib.tok_triplet_fwd(X, X, X, rows, c, ld, 0.3, 1e-6, 0, ds, rt, l3, st), 'triplet_fwd')
        ok(lib.tok_triplet_bwd(X, X, X, V3, G, rows, c, ld, 0.3, 1e-6, 0, ta, tp, tn, st), 'triplet_bwd')
        sm, tv, ti = new(sq, lambda: Mat(rows, 3, dtype=F32), lambda: Mat(rows, 3, dtype=I64))
        ok(lib.tok_sim_matrix(XF, XF, rows, rows, c, ld, ld, 0, sm, rows, st), 'sim_matrix')
        ok(lib.tok_topk_rows(RR, rows, rows, rows, 3, tv, ti, st), 'topk_rows')
        nr_, ev_ = new(lambda: vec_out(rows, I32), v1)
        ok(lib.tok_retrieval_nrel(L, None, rows, 0, L, None, rows, nr_, st), 'retrieval_nrel')
        ok(lib.tok_retrieval_eval(0, IX, 3, U, None, rows, L, None, 0, L, None, N32, None, rows, ev_, st), 'retrieval_eval')
        return [bits(m) for m in ms]
    first = valid()

    # every NULL operand
    _null_each(lib.tok_l2norm_fwd, (X, b0, f0, rows, c, ld, 0, 1e-12, st), (0, 1, 2), 'l2norm_fwd')
    _null_each(lib.tok_l2norm_bwd, (X, X, V, b0, 0, rows, c, ld, 0, st), (0, 1, 2, 3), 'l2norm_bwd')
    _null_each(lib.tok_arcface_margin_fwd, (X, T_, rows, c, ld, *arc, b0, st), (0, 1, 11), 'arcface_fwd')
    _null_each(lib.tok_arcface_margin_bwd, (X, T_, X, rows, c, ld, *arc, b0, st), (0, 1, 2, 12), 'arcface_bwd')
    _null_each(lib.tok_relevance_matrix, (L, L, rows, rows, f0, st), (0, 1, 4), 'relevance')
    _null_each(lib.tok_relevance_matrix_multilabel, (XF, XF, rows, rows, c, f0, st), (0, 1, 5), 'relevance_ml')
    _null_each(lib.tok_contrastive_fwd, (X, X, RR, rows, rows, c, ld, 1.0, f0, f1, lo, st), (0, 1, 2, 8, 9, 10), 'contrastive_fwd')
    _null_each(lib.tok_contrastive_bwd, (X, X, RR, SS, G, rows, rows, c, ld, 1.0, b0, b1, 0, st), (0, 1, 2, 3, 10, 11), 'contrastive_bwd')
    _null_each(lib.tok_embed_reg_fwd, (X, rows, c, ld, 1, f0, lo, st), (0, 5, 6), 'embed_reg_fwd')
    _null_each(lib.tok_embed_reg_bwd, (X, V, G, 0.1, rows, c, ld, 1, b0, st), (0, 1, 2, 8), 'embed_reg_bwd')
    _null_each(lib.tok_ntxent_fwd, (X, 4, c, ld, 0.5, f0, f1, lo, st), (0, 5, 6, 7), 'ntxent_fwd')
    _null_each(lib.tok_ntxent_bwd, (X, V, G, 4, c, ld, 0.5, b0, st), (0, 1, 7), 'ntxent_bwd')
    _null_each(lib.tok_triplet_fwd, (X, X, X, rows, c, ld, 0.3, 1e-6, 0, f0, f1, lo, st), (0, 1, 2, 9, 10, 11), 'triplet_fwd')
    _null_each(lib.tok_triplet_bwd, (X, X, X, V3, G, rows, c, ld, 0.3, 1e-6, 0, b0, b1, b2, st), (0, 1, 2, 3, 11, 12, 13), 'triplet_bwd')
    _null_each(lib.tok_sim_matrix, (XF, XF, rows, rows, c, ld, ld, 0, f0, rows, st), (0, 1, 8), 'sim_matrix')
    _null_each(lib.tok_topk_rows, (RR, rows, rows, rows, 3, f0, o64, st), (0, 5, 6), 'topk_rows')
    _null_each(lib.tok_retrieval_nrel, (L, None, rows, 0, L, None, rows, o32, st), (0, 4, 7), 'nrel (labels)')
    _null_each(lib.tok_retrieval_nrel, (None, XF, rows, ld, None, L, rows, o32, st), (1, 5, 7), 'nrel (scores)')
    ev = (0, IX, 3, U, None, rows, L, None, 0, L, None, N32, None, rows, f0, st)
    _null_each(lib.tok_retrieval_eval, ev, (1, 3, 6, 9, 11, 14), 'eval (labels)')
    evs = (0, IX, 3, U, None, rows, None, XF, ld, L, L, N32, None, rows, f0, st)
    _null_each(lib.tok_retrieval_eval, evs, (1, 3, 7, 9, 10, 11, 14), 'eval (scores)')

    # ld < c, zero sizes
    for r_, c_, l_ in ((rows, c, c - 1), (0, c, ld), (rows, 0, ld)):
        _refused(lib.tok_l2norm_fwd(X, b0, f0, r_, c_, l_, 0, 1e-12, st), 'l2norm_fwd size')
        _refused(lib.tok_l2norm_bwd(X, X, V, b0, 0, r_, c_, l_, 0, st), 'l2norm_bwd size')
        _refused(lib.tok_arcface_margin_fwd(X, T_, r_, c_, l_, *arc, b0, st), 'arcface_fwd size')
        _refused(lib.tok_arcface_margin_bwd(X, T_, X, r_, c_, l_, *arc, b0, st), 'arcface_bwd size')
        _refused(lib.tok_contrastive_fwd(X, X, RR, r_, rows, c_, l_, 1.0, f0, f1, lo, st), 'contrastive_fwd size')
        _refused(lib.tok_contrastive_bwd(X, X, RR, SS, G, r_, rows, c_, l_, 1.0, b0, b1, 0, st), 'contrastive_bwd size')
        _refused(lib.tok_embed_reg_fwd(X, r_, c_, l_, 1, f0, lo, st), 'embed_reg_fwd size')
        _refused(lib.tok_embed_reg_bwd(X, V, G, 0.1, r_, c_, l_, 1, b0, st), 'embed_reg_bwd size')
        _refused(lib.tok_ntxent_fwd(X, 4 if r_ else 0, c_, l_, 0.5, f0, f1, lo, st), 'ntxent_fwd size')
        _refused(lib.tok_ntxent_bwd(X, V, G, 4 if r_ else 0, c_, l_, 0.5, b0, st), 'ntxent_bwd size')
        _refused(lib.tok_triplet_fwd(X, X, X, r_, c_, l_, 0.3, 1e-6, 0, f0, f1, lo, st), 'triplet_fwd size')
        _refused(lib.tok_triplet_bwd(X, X, X, V3, G, r_, c_, l_, 0.3, 1e-6, 0, b0, b1, b2, st), 'triplet_bwd size')
        _refused(lib.tok_sim_matrix(XF, XF, r_, rows, c_, l_, ld, 0, f0, rows, st), 'sim_matrix size (q)')
        _refused(lib.tok_sim_matrix(XF, XF, rows, r_, c_, ld, l_, 0, f0, rows, st), 'sim_matrix size (g)')
    _refused(lib.tok_contrastive_fwd(X, X, RR, rows, 0, c, ld, 1.0, f0, f1, lo, st), 'contrastive_fwd n2 = 0')
    _refused(lib.tok_sim_matrix(XF, XF, rows, rows, c, ld, ld, 0, f0, rows - 1, st), 'sim_matrix ldo < ng')
    _refused(lib.tok_relevance_matrix(L, L, 0, rows, f0, st), 'relevance na = 0')
    _refused(lib.tok_relevance_matrix_multilabel(XF, XF, rows, 0, c, f0, st), 'relevance_ml nb = 0')
    _refused(lib.tok_relevance_matrix_multilabel(XF, XF, rows, rows, 0, f0, st), 'relevance_ml classes = 0')
    for r_, c_, l_, k_ in ((0, rows, rows, 3), (rows, 0, rows, 3), (rows, rows, rows - 1, 3), (rows, rows, rows, 0)):
        _refused(lib.tok_topk_rows(RR, r_, c_, l_, k_, f0, o64, st), 'topk_rows size')
    _refused(lib.tok_retrieval_nrel(L, None, 0, 0, L, None, rows, o32, st), 'nrel n = 0')
    _refused(lib.tok_retrieval_nrel(L, None, rows, 0, L, None, 0, o32, st), 'nrel nq = 0')
    _refused(lib.tok_retrieval_nrel(None, XF, rows, 0, None, L, rows, o32, st), 'nrel n_cols = 0')
    # NT-Xent: n odd, n < 2, temperature <= 0; the backward's register file: d = 1025, ld = 1032
    big = z(4, 1032)
    for n_ in (3, 5, 1):
        _refused(lib.tok_ntxent_fwd(X, n_, c, ld, 0.5, f0, f1, lo, st), 'ntxent_fwd n odd')
        _refused(lib.tok_ntxent_bwd(X, V, G, n_, c, ld, 0.5, b0, st), 'ntxent_bwd n odd')
    _refused(lib.tok_ntxent_fwd(X, 4, c, ld, 0.0, f0, f1, lo, st), 'ntxent_fwd T = 0')
    _refused(lib.tok_ntxent_bwd(P(big), V, G, 4, 1025, 1032, 0.5, outs['f6'].ptr, st), 'ntxent_bwd d = 1025')
    _refused(lib.tok_ntxent_bwd(P(big), V, G, 4, 1024, 1032, 0.5, outs['f6'].ptr, st), 'ntxent_bwd ld = 1032')
    # mode, metric, kind, labels / scores both or neither, kk < 2
    for mode in (0, 3):
        _refused(lib.tok_embed_reg_fwd(X, rows, c, ld, mode, f0, lo, st), 'embed_reg_fwd mode')
        _refused(lib.tok_embed_reg_bwd(X, V, G, 0.1, rows, c, ld, mode, b0, st), 'embed_reg_bwd mode')
    for metric in (-1, 2):
        _refused(lib.tok_sim_matrix(XF, XF, rows, rows, c, ld, ld, metric, f0, rows, st), 'sim_matrix metric')
    for kind in (-1, 5):
        _refused(lib.tok_retrieval_eval(kind, *ev[1:]), 'eval kind')
    _refused(lib.tok_retrieval_nrel(L, XF, rows, ld, L, L, rows, o32, st), 'nrel labels and scores')
    _refused(lib.tok_retrieval_nrel(None, None, rows, ld, L, L, rows, o32, st), 'nrel neither')
    _refused(lib.tok_retrieval_eval(0, IX, 3, U, None, rows, L, XF, ld, L, L, N32, None, rows, f0, st), 'eval labels and scores')
    _refused(lib.tok_retrieval_eval(0, IX, 3, U, None, rows, None, None, ld, L, L, N32, None, rows, f0, st), 'eval neither')
    _refused(lib.tok_retrieval_eval(0, IX, 1, U, None, rows, L, None, 0, L, None, N32, None, rows, f0, st), 'eval kk < 2')
    _refused(lib.tok_retrieval_eval(0, IX, 3, U, None, 0, L, None, 0, L, None, N32, None, rows, f0, st), 'eval ng = 0')
    _refused(lib.tok_retrieval_eval(0, IX, 3, U, None, rows, L, None, 0, L, None, N32, None, 0, f0, st), 'eval nq = 0')
    # suspect 1: one tensor, n1 != n2 (in both directions)
    _refused(lib.tok_contrastive_bwd(X, X, RR, SS, G, rows, 3, c, ld, 1.0, b0, None, 1, st), 'contrastive_bwd same tensor, n2 < n1')
    assert 'n1 == n2' in last_error()
    _refused(lib.tok_contrastive_bwd(X, X, RR, SS, G, 3, rows, c, ld, 1.0, b0, None, 1, st), 'contrastive_bwd same tensor, n2 > n1')
    # suspect 2: na * nb past 2^31 - 1 wrapped the int index and the grid; 46341^2 = 2^31 + 4633 is the first square past it
    for na, nb in ((65536, 32768), (46341, 46341), (2 ** 31 - 1, 2)):
        _refused(lib.tok_relevance_matrix(L, L, na, nb, f0, st), f'relevance {na} x {nb}')
        assert '2^31 - 1' in last_error()
        _refused(lib.tok_relevance_matrix_multilabel(XF, XF, na, nb, c, f0, st), f'relevance_ml {na} x {nb}')
    torch.cuda.synchronize()
    for ms in outs.values():
        for m_ in (ms if isinstance(ms, list) else [ms]):
            if isinstance(m_, Mat):
                m_.intact('an output of refused calls')
            else:
                m_.check('loss')
                assert m_.untouched(), 'loss written by a refused call'
    again = valid()
    assert all(torch.equal(a, b) for a, b in zip(first, again)), 'a valid call after the refusals differs from the one before'
