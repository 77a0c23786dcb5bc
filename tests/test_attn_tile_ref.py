"""tests/attn_tile_ref.py on the CPU: the hand-written fp64 backward against torch's autograd of a plain softmax(Q K^T s + bias) V,
both addressings against their inverses, the input makers against what they claim, the restatement of dbias_per_chunk against the
counts the existing GPU modules assert, and the bounds against an fp32 emulation of the kernels' rounding points: it passes, and
each of four defects does not."""
import math

import pytest
import torch

import attn_tile_ref as R

F64 = torch.float64


def _close(a, b, tol=1e-11):
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max()) / scale


@pytest.mark.parametrize('hd,n,biased,shared', [(64, 5, False, False), (64, 70, True, False), (32, 9, True, False),
                                                (32, 81, True, True)])
def test_reference_is_autograd_of_plain_attention(hd, n, biased, shared):
    units, uq = (6, 3) if shared else (3, 3)
    q, k, v, dout, bias = R.make('random', units, 2, n, hd, seed=n, biased=biased, uq=uq)
    qimg = R.query_image(units, uq) if shared else None
    ref = R.Ref(q, k, v, dout, bias, qimg, 'windowed' if hd == 32 else 'dense')
    out, lse, dq, dk, dv, dbias = R.autograd(q, k, v, dout, bias, qimg)
    _close(ref.out, out)
    _close(ref.lse, lse)
    _close(ref.dq_global if shared else ref.dq, dq)
    _close(ref.dk, dk)
    _close(ref.dv, dv)
    if biased:
        _close(ref.dbias, dbias)
    else:
        assert ref.dbias is None and 'dbias' not in ref.bounds
    for name in ref.bounds:
        b = ref.bound(name)
        assert torch.isfinite(b).all() and (b > 0).all(), name


def test_addressing_round_trips():
    b, n, heads = 2, 5, 3
    rows = torch.arange(b * n * 3 * heads * 64, dtype=F64).reshape(b * n, -1)
    q, k, v = R.dense_units(rows, b, n, heads, 3)
    assert q.shape == (b, heads, n, 64) and float(k[1, 2, 3, 4]) == float(rows[1 * n + 3, (heads + 2) * 64 + 4])
    assert torch.equal(R.dense_rows(q, k, v), rows)
    geo = (3, 4, 6, 2, 2)                                     # B 3, 4 x 6 map, 2 heads, ws 2: nW = 2 x 3
    rows = torch.arange(3 * 24 * 2 * 2 * 32, dtype=F64).reshape(72, -1)
    kk, vv = R.window_units(rows, geo, 2)
    assert kk.shape == (18, 2, 4, 32)
    # window 7 = image 1, wy 0, wx 1; its token 3 = (row 1, column 1) of the window = map position (1, 3)
    assert float(vv[7, 1, 3, 5]) == float(rows[24 + 1 * 6 + 3, (2 + 1) * 32 + 5])
    assert torch.equal(R.window_rows(geo, kk, vv), rows)
    assert R.query_image(6, 3).tolist() == [0, 1, 2, 0, 1, 2]


def test_chunk_restatement_gives_the_counts_the_gpu_modules_assert():
    assert R.dbias_chunks(70, 5, 1, 64) == (2, 35)
    assert R.dbias_chunks(3, 5, 2, 64) == (1, 3)
    assert R.dbias_chunks(130, 65, 1, 64) == (3, 44)
    assert R.dbias_chunks(256, 197, 12, 64)[1] == 11
    assert R.dbias_chunks(256 * 64, 49, 2, 128)[1] == 128
    assert R.dbias_chunks(1, 4096, 1, 64) == (1, 1)


def _softmax(q, k, bias, hd):
    s = (q.double() @ k.double().transpose(-2, -1)) * R.SCALE[hd]
    return s, (s if bias is None else s + bias.double())


@pytest.mark.parametrize('hd,n', [(64, 193), (32, 144)])
def test_input_makers_produce_what_they_claim(hd, n):
    units, heads = 2, 2
    nt = R.cdiv(n, R.TL)
    for biased in (False, True):
        for kind, key in (('max_last', n - 1), ('max_first', 0)):
            q, k, v, dout, bias = R.make(kind, units, heads, n, hd, 3, biased)
            _, s = _softmax(q, k, bias, hd)
            assert (s.argmax(-1) == key).all()
            top = s.max(-1).values.unsqueeze(-1)
            rest = torch.where(torch.arange(n) == key, -math.inf, 0.0) + s
            assert (top - rest.max(-1, keepdim=True).values > 100).all()      # one-hot rows ...
            assert (s.softmax(-1).amax(-1) > 1 - 1e-12).all()
        q, k, v, dout, bias = R.make('max_first', units, heads, n, hd, 3, False)
        _, s = _softmax(q, k, None, hd)
        assert (s[..., 0:1] - s[..., R.TL:] > 100).all()                       # ... every later tile more than 100 nats below key 0
        q, k, v, dout, bias = R.make('alternate', units, heads, n, hd, 3, biased)
        _, s = _softmax(q, k, bias, hd)
        assert (s.argmax(-1) == R.alternate_key(n)).all()
        tiles = R.alternate_key(n) // R.TL
        assert (tiles[1:] != tiles[:-1]).all() and set(tiles.tolist()) == set(range(nt))
        # the running maximum of a row moves by a few nats, not by ~100: alpha is neither 0 nor 1 in the tiles before the peak
        run = torch.stack([s[..., :min((t + 1) * R.TL, n)].amax(-1) for t in range(nt)], -1)
        step = run[..., 1:] - run[..., :-1]
        assert float(step.max()) < 12 and float((step > 0.05).double().mean()) > 0.3
    q, k, v, dout, bias = R.make('bias_decides', units, heads, n, hd, 3, True)
    qk, s = _softmax(q, k, bias, hd)
    assert (qk.argmax(-1) == 0).all() and (s.argmax(-1) == R.decided_key(n)).all()
    assert float(bias.abs().max()) > 95 and (qk[..., 0] - qk[..., 1:].amax(-1) > 15).all()
    for kind, first in (('tile_masked', False), ('first_tile_masked', True)):
        q, k, v, dout, bias = R.make(kind, units, heads, n, hd, 3, True)
        lo, hi = R.masked_tile(n, first)
        assert (lo == 0) == first and hi - lo == R.TL
        masked = bias <= -1e4
        assert masked[:, R.masked_rows(n), lo:hi].all()
        share = float(masked.double().mean())
        assert share == pytest.approx(float(R.masked_rows(n).double().mean()) * R.TL / n)
        p = _softmax(q, k, bias, hd)[1].softmax(-1)
        assert float(p[masked.expand_as(p)].max()) == 0.0 and torch.isfinite(torch.logsumexp(_softmax(q, k, bias, hd)[1], -1)).all()
    q, k, v, dout, bias = R.make('row_masked', units, heads, n, hd, 3, True)
    lse = torch.logsumexp(_softmax(q, k, bias, hd)[1], -1)
    assert (lse[..., R.masked_rows(n)] < -2.9e4).all() and (lse[..., ~R.masked_rows(n)].abs() < 50).all()
    assert (bias[:, R.masked_rows(n)] < -2.9e4).all() and float((bias < -1e4).double().mean()) == float(R.masked_rows(n).double().mean())
    assert (2.0 ** 127 < torch.exp2(-lse[..., R.masked_rows(n)] * 1.4426950408889634)).all()      # past fp32: exp2f gives inf
    q, k, v, dout, bias = R.make('uniform', units, heads, n, hd, 3, True)
    ref = R.Ref(q, k, v, dout, bias, None, 'dense')
    _close(ref.lse, torch.full_like(ref.lse, math.log(n)))
    _close(ref.out, v.double().mean(2, keepdim=True).expand_as(ref.out))
    q, k, v, dout, bias = R.make('dout_zero', units, heads, n, hd, 3, True)
    assert not dout.any()
    q, k, v, dout, bias = R.make('dout_one_row', units, heads, n, hd, 3, True)
    nz = dout.float().abs().sum(-1).nonzero().tolist()
    assert nz == [[0, heads - 1, n // 2]]


@pytest.mark.parametrize('kind', ['random', 'max_last', 'alternate', 'tile_masked', 'row_masked'])
@pytest.mark.parametrize('hd,n,family', [(64, 130, 'dense'), (32, 81, 'windowed')])
def test_bounds_admit_the_rounding_points_and_refuse_defects(hd, n, family, kind):
    units, heads = 4, 2
    q, k, v, dout, bias = R.make(kind, units, heads, n, hd, 11, True)
    ref = R.Ref(q, k, v, dout, bias, None, family)
    worst = ref.check(R.emulate(q, k, v, dout, bias, None, family))
    assert max(worst.values()) <= 1.0
    if kind != 'random':
        return
    caught = {}
    for variant, names in (('extra_key', ('lse',)), ('no_alpha', ('lse',)), ('scale32', ('lse', 'dq')),
                           ('dbias_bf16', ('dbias',))):
        if variant == 'dbias_bf16' and family == 'dense':
            continue          # the dense bound of dbias holds the bf16 rounding of the stored O (through delta): same size
        res = R.emulate(q, k, v, dout, bias, None, family, variant)
        caught[variant] = {nm: ref.ratio(nm, res[nm]) for nm in names}
        assert all(r > 1.0 for r in caught[variant].values()), caught
    # the shared query: the bound of d(q_global) adds up the windows'
    qs, k, v, dout, bias = R.make('random', units, heads, n, hd, 12, True, uq=2)
    qimg = R.query_image(units, 2)
    ref = R.Ref(qs, k, v, dout, bias, qimg, family)
    ref.check(R.emulate(qs, k, v, dout, bias, qimg, family))


def test_uniform_rows_bound_of_lse_is_a_few_ulps():
    q, k, v, dout, bias = R.make('uniform', 1, 1, 100, 64, 1, False)
    ref = R.Ref(q, k, v, dout)
    b = ref.bound('lse')
    assert float(b.max()) < 16 * 2.0 ** -24 * math.log(100) and float(b.min()) > 2 * 2.0 ** -24 * math.log(100)
