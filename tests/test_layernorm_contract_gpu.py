"""tok_layernorm_fwd / _bwd (csrc/layernorm.hip: ln_*_vec_kernel<LPR, VPL> and the one-wave-per-row fallback) element by
element against fp64 of the same bf16 inputs; the bounds are derived in tests/layernorm_ref.py.  Widths on both sides of every
dispatch boundary (c / 8 <= 16 / 32 / 64 / else, the fallback at c != ld, c % 8 and c > 1024), row counts that leave partial
waves for every lanes-per-row, a row count over the backward's grid cap (grid-stride loop and second row slot), with and
without shortcut / row_scale (one sample scaled by 0), accumulate 0 and 1, and in every case of five rows or more a constant
row (variance 0), a row 64 + 0.5 noise and a zero row.  Guard rows hold sentinels; the fallback zeroes the pad columns."""
import pytest
import torch

from helpers import F32, SENTINEL, Guarded, _INT_OF
from layernorm_ref import EPS, LNRef, check_bwd, check_fwd, make_inputs
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
P = lambda t: None if t is None else t.data_ptr()       # noqa: E731


def _owned(g, what, zero_pads):
    iv = g.buf.view(_INT_OF[g.dtype])
    assert int((iv[:g.rows, :g.cols] == SENTINEL[g.dtype]).sum()) == 0, f'{what}: owned elements never written'
    assert torch.isfinite(g.view.float()).all(), what
    assert bool((iv[g.rows] == SENTINEL[g.dtype]).all()), f'{what}: guard row overwritten'
    if zero_pads:
        assert bool((g.buf[:g.rows, g.cols:] == 0).all()), f'{what}: pad columns are not zero'
    else:
        g.check(what)


def _run(tag, rows, c, ld, sc, rs, seed, pair=False):
    lib, st = _C.lib(), stream_ptr()
    d = make_inputs(rows, c, sc, rs, seed)
    ref = LNRef(d)
    fallback = not (c == ld and c % 8 == 0 and c <= 1024)
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items()}
    xg = Guarded(rows, c, ld, init=dev['x'], nan_pad=True)
    hg = Guarded(rows, c, ld, init=dev['shortcut'], nan_pad=True) if sc else None
    og = Guarded(rows, c, ld)
    mg, rg = Guarded(1, rows, dtype=F32), Guarded(1, rows, dtype=F32)
    _C.check(lib.tok_layernorm_fwd(xg.ptr, hg.ptr if sc else None, P(dev['row_scale']), d['rps'], P(dev['gamma']), P(dev['beta']),
                                   og.ptr, mg.ptr, rg.ptr, rows, c, ld, EPS, st), 'fwd')
    torch.cuda.synchronize()
    xg.check('x')
    _owned(og, 'out', fallback and ld > c)
    _owned(mg, 'mean', False)
    _owned(rg, 'rstd', False)
    check_fwd(tag, ref, og.value(), mg.value()[0], rg.value()[0])
    # backward, alone: fed the fp32-rounded fp64 statistics
    r = lib.tok_layernorm_bwd_rows(rows, c)
    assert r == min((rows + 3) // 4, 1024), f'{r} partial rows: has tok_layernorm_bwd_rows (csrc/layernorm.hip) left its cap of 1024?'
    gg = Guarded(rows, c, ld, init=dev['dout'], nan_pad=True)
    m32, r32 = ref.mean32.cuda(), ref.rstd32.cuda()
    for acc in (0, 1):
        dg = Guarded(rows, c, ld, init=dev['dx0'] if acc else None)
        pg = Guarded(2 * r, c, dtype=F32)
        _C.check(lib.tok_layernorm_bwd(gg.ptr, xg.ptr, P(m32), P(r32), P(dev['gamma']), P(dev['row_scale']), d['rps'], dg.ptr, acc,
                                       pg.ptr, rows, c, ld, st), 'bwd')
        torch.cuda.synchronize()
        gg.check('dout')
        _owned(dg, 'dx', fallback and ld > c)
        _owned(pg, 'partial', False)
        part = pg.value().double().view(2, r, c)
        check_bwd(tag, ref, acc, dg.value(), part[0].sum(0), part[1].sum(0))
        if pair and acc:
            fg = Guarded(2, c, dtype=F32)
            fg.view.fill_(1.0)
            _C.check(lib.tok_colsum_f32_pair(pg.ptr, pg.ptr + 4 * r * c, r, c, fg.ptr, 0, fg.ptr + 4 * c, 1, st), 'pair fold')
            torch.cuda.synchronize()
            fg.check('folded')
            f = fg.value().double()
            f[1] -= 1.0                                       # the second fold accumulated onto ones
            check_bwd(tag + '_pairfold', ref, acc, dg.value(), f[0], f[1])
    return d, ref, og.value(), rg.value()[0]


# (c, ld): LPR 16 / 32 / 64 and VPL 2 on both sides of each boundary, then the fallback (c > 1024, c % 8, c != ld)
WIDTHS = [(8, 8), (128, 128), (136, 136), (256, 256), (264, 264), (512, 512), (520, 520), (1024, 1024),
          (1032, 1032), (100, 104), (96, 104)]


@pytest.mark.parametrize('c,ld', WIDTHS)
def test_widths_and_partial_waves(c, ld):
    for rows, sc, rs in ((1, 0, 0), (5, 1, 0), (17, 0, 1), (33, 1, 1)):
        d, ref, out, rstd = _run(f'layernorm_contract/c{c}_ld{ld}_r{rows}', rows, c, ld, sc, rs, seed=c + rows, pair=(rows == 33))
        if rows >= 5:
            # the constant rows: rstd = eps^-1/2 and the output is beta * row_scale + shortcut
            for row in (0, 2):
                assert abs(float(rstd[row]) - EPS ** -0.5) <= 2.0 ** -20 * EPS ** -0.5
            assert float(ref.rstd[0]) == EPS ** -0.5
            # ... directly, to one bf16 ulp (2^-7 relative): x - mean must vanish, whatever the generic bound would let through
            bs, sh = (d['beta'].double() * ref.sc)[[0, 2]], ref.sh[[0, 2]]       # (+ 2^-20 of the two terms: their fp32 sum)
            assert ((out[[0, 2]].double() - (bs + sh)).abs() <= 2.0 ** -7 * (bs + sh).abs() + 2.0 ** -20 * (bs.abs() + sh.abs())).all()


def test_row_count_over_the_backward_grid_cap():
    """4096 x 16 + 19 rows at c = 8 (16 rows per block pass): more than 1024 blocks x 2 row slots, so the grid-stride loop
    runs three times, the last time with a partly empty first slot and an empty second one"""
    _run('layernorm_contract/cap_c8', 4096 * 16 + 19, 8, 8, 1, 1, seed=7, pair=True)
