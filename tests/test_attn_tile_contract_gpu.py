"""The six entry points that run the kernel text of csrc/attn_tile.h (tok_global_attn_fwd / _bwd, tok_global_attn_bias_fwd / _bwd,
tok_gc_attn_fwd / _bwd) at the edges of its 64-token tiles, 16-query waves and 4-key bias groups: every token count and window
size at which a tile, a wave or a group straddles N, logits built to move the running maximum of the online softmax in every way
it can move, the largest grids admitted, and the identities between the families.

Every case runs on guarded buffers (NaN input pads and guards, sentinel outputs, a workspace of exactly *_ws_bytes behind a
guard), runs twice with all outputs compared bit for bit, and is compared element by element with the fp64 reference of
tests/attn_tile_ref.py, whose docstring derives every bound from the rounding points of the kernels.  No element is excluded
from any comparison.  The worst |err| / bound of every tensor is recorded (helpers.record_distance, folded into
profiles/attn_tile_contract_parity_distances.json); profiles/attn_tile_contract_mutation_check.txt lists the one-line kernel
defects each of these tests was seen to catch."""
import math

import pytest
import torch

import attn_tile_ref as R
import test_gc_attn_contract_gpu as G
from helpers import ERR_INVALID, Guarded, GuardedSpan, last_error, record_distance
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
U32 = 2.0 ** -24
DENSE_MAX_CHUNKS, WINDOW_MAX_CHUNKS = 64, 128


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(first, again, what):
    assert first.keys() == again.keys()
    for name in first:
        x, y = first[name], again[name]
        assert (x is None and y is None) or torch.equal(_bits(x), _bits(y)), f'{what}: {name} differs between two runs'


def _record(tag):
    def rec(worst):
        print(tag, {k: round(v, 4) for k, v in worst.items()})
        for k, v in worst.items():
            record_distance('attn_tile_contract/' + tag, k, err_over_bound=v)
    return rec


def _ldb(n):
    return (n + 3) // 4 * 4 + 4


def _ceil4(n):
    return (n + 3) // 4 * 4


# ---- launchers -------------------------------------------------------------------------------------------------------------------
def _dense_once(q, k, v, dout, bias, ldb, dbias_mode, prior):
    """forward + backward of the dense family in the unit layout; bias None: the un-biased entries"""
    lib, st = _C.lib(), stream_ptr()
    b, heads, n, hd = k.shape
    c = heads * hd
    ldq, ldo, ldd = 3 * c + 8, c + 24, 3 * c + 16
    qg = Guarded(b * n, 3 * c, ldq, init=R.dense_rows(q, k, v).cuda(), nan_pad=True)
    gg = Guarded(b * n, c, ldo, init=R.dense_rows(dout).cuda(), nan_pad=True)
    og, lg, dg = Guarded(b * n, c, ldo), Guarded(b * heads, n, dtype=F32), Guarded(b * n, 3 * c, ldd)
    dbg = None
    if bias is None:
        _C.check(lib.tok_global_attn_fwd(qg.ptr, ldq, b, n, heads, hd, og.ptr, ldo, lg.ptr, st), 'fwd')
        ws_bytes = lib.tok_global_attn_bwd_ws_bytes(b, n, heads)
        wsg = GuardedSpan(ws_bytes, torch.uint8, 4096, nan_guard=True)
        _C.check(lib.tok_global_attn_bwd(qg.ptr, ldq, og.ptr, gg.ptr, ldo, lg.ptr, b, n, heads, hd, dg.ptr, ldd, wsg.ptr, ws_bytes,
                                         st), 'bwd')
    else:
        bg = torch.full((heads * n + 1, ldb), float('nan'), dtype=F32, device='cuda')
        bg[:heads * n, :n] = bias.reshape(heads * n, n).cuda()
        _C.check(lib.tok_global_attn_bias_fwd(qg.ptr, ldq, bg.data_ptr(), ldb, b, n, heads, hd, og.ptr, ldo, lg.ptr, st), 'fwd')
        dbg = Guarded(heads * n, n, ldb, dtype=F32, init=None if prior is None else prior.cuda())
        want = dbias_mode != 'none'
        ws_bytes = lib.tok_global_attn_bias_bwd_ws_bytes(b, n, heads, ldb) if want else lib.tok_global_attn_bwd_ws_bytes(b, n, heads)
        wsg = GuardedSpan(ws_bytes, torch.uint8, 4096, nan_guard=True)
        _C.check(lib.tok_global_attn_bias_bwd(qg.ptr, ldq, og.ptr, gg.ptr, ldo, lg.ptr, bg.data_ptr(), ldb, b, n, heads, hd, dg.ptr,
                                              ldd, dbg.ptr if want else None, int(dbias_mode == 'add'), wsg.ptr, ws_bytes, st), 'bwd')
    torch.cuda.synchronize()
    for buf, what in ((qg, 'qkv'), (gg, 'dout'), (og, 'out'), (lg, 'lse'), (dg, 'dqkv'), (wsg, 'ws'), (dbg, 'dbias')):
        if buf is not None:
            buf.check(what)
    res = {'out': R.dense_units(og.value(), b, n, heads, 1)[0], 'lse': lg.value().view(b, heads, n)}
    res['dq'], res['dk'], res['dv'] = R.dense_units(dg.value(), b, n, heads, 3)
    res['dbias'] = None
    if bias is not None:
        assert torch.isnan(bg[:heads * n, n:]).all() and torch.isnan(bg[heads * n]).all()
        if dbias_mode == 'none':
            assert bool((_bits(dbg.view) == dbg.bits).all()), 'a NULL dbias was written'
        else:
            res['dbias'] = dbg.value().view(heads, n, n)
    return res


def _dense(q, k, v, dout, bias=None, ldb=None, dbias_mode='set', prior=None, what='dense'):
    ldb = _ldb(k.shape[2]) if ldb is None else ldb
    first = _dense_once(q, k, v, dout, bias, ldb, dbias_mode, prior)
    _same_bits(first, _dense_once(q, k, v, dout, bias, ldb, dbias_mode, prior), what)
    return first


def _window_once(geo, q, k, v, dout, bias, shared, dbias_mode, prior):
    b, h, w, heads, ws = geo
    n = ws * ws
    if shared:
        rows, qg = R.window_rows(geo, k, v), R.dense_rows(q)
    else:
        rows, qg = R.window_rows(geo, q, k, v), None
    out, lse, dqkv, dqg, dbias = G._launch(geo, rows, qg, bias, R.window_rows(geo, dout), dbias_mode, prior)
    res = {'out': R.window_units(out, geo, 1)[0], 'lse': lse, 'dbias': dbias}
    if shared:
        res['dk'], res['dv'] = R.window_units(dqkv, geo, 2)
        res['dq_global'] = R.dense_units(dqg, b, n, heads, 1, hd=32)[0]
    else:
        res['dq'], res['dk'], res['dv'] = R.window_units(dqkv, geo, 3)
    return res


def _window(geo, q, k, v, dout, bias, shared, dbias_mode='set', prior=None, what='windowed'):
    first = _window_once(geo, q, k, v, dout, bias, shared, dbias_mode, prior)
    _same_bits(first, _window_once(geo, q, k, v, dout, bias, shared, dbias_mode, prior), what)
    return first


def _window_chunks(geo):
    b, h, w, heads, ws = geo
    return R.dbias_chunks(b * (h // ws) * (w // ws), ws * ws, heads, WINDOW_MAX_CHUNKS)


def _window_ref(geo, q, k, v, dout, bias, shared):
    units = k.shape[0]
    return R.Ref(q, k, v, dout, bias, R.query_image(units, geo[0]) if shared else None, 'windowed', _window_chunks(geo)[1])


def _accumulated(acc, prior, first):
    want = prior.double() + first.double()
    assert ((acc.double() - want).abs() <= U32 * want.abs() + 1e-45).all()       # one fp32 rounding of the sum


# ---- token-count sweep, dense family -------------------------------------------------------------------------------------------
# below a wave, at and around a wave (16), a tile (64), two tiles and three; with b = 2 image 0's tail tile is followed in memory
# by image 1's live rows
DENSE_N = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 193]


@pytest.mark.parametrize('n', DENSE_N)
def test_dense_token_counts(n):
    b, heads = 2, 2
    q, k, v, dout, bias = R.make('random', b, heads, n, 64, seed=n, biased=True)
    plain = _dense(q, k, v, dout, what='plain')
    R.Ref(q, k, v, dout).check({x: plain[x] for x in ('out', 'lse', 'dq', 'dk', 'dv')}, _record('dense_plain/n%d' % n))
    chunks = R.dbias_chunks(b, n, heads, DENSE_MAX_CHUNKS)[1]
    assert _C.lib().tok_global_attn_bias_bwd_chunks(b, n, heads) == chunks
    ref = R.Ref(q, k, v, dout, bias, chunks=chunks)
    results = {}
    # the pitch of the other modules, and the smallest legal one: the float4 of the last key group ends exactly at the row end
    for ldb in (_ldb(n), _ceil4(n)):
        results[ldb] = _dense(q, k, v, dout, bias, ldb, what='biased ldb %d' % ldb)
        ref.check(results[ldb], _record('dense_biased/n%d_ldb%d' % (n, ldb)))
    _same_bits(results[_ldb(n)], results[_ceil4(n)], 'the bias pitch')
    # zero bias: the bits of the un-biased entries
    zero = _dense(q, k, v, dout, torch.zeros(heads, n, n), _ceil4(n), what='zero bias')
    _same_bits(plain, dict(zero, dbias=None), 'zero bias against the un-biased entry')


@pytest.mark.parametrize('n', [5, 65, 129])
def test_dense_dbias_modes(n):
    b, heads = 2, 2
    q, k, v, dout, bias = R.make('random', b, heads, n, 64, seed=100 + n, biased=True)
    first = _dense(q, k, v, dout, bias)
    none = _dense(q, k, v, dout, bias, dbias_mode='none')
    _same_bits(dict(first, dbias=None), none, 'dbias == NULL')
    prior = torch.randn(heads, n, n, generator=torch.Generator().manual_seed(5))
    acc = _dense(q, k, v, dout, bias, dbias_mode='add', prior=prior)
    _accumulated(acc['dbias'], prior, first['dbias'])


# ---- window-size sweep, windowed family ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shared', [False, True], ids=['local', 'global'])
@pytest.mark.parametrize('ws', list(range(1, 17)))
def test_window_sizes(ws, shared):
    """N = 1 ... 256 on the smallest map with two windows per image; batch 3 and 2 windows per image, so u % batch != u / nW"""
    geo = (3, ws, 2 * ws, 2, ws)
    b, heads, n = 3, 2, ws * ws
    q, k, v, dout, bias = R.make('random', 6, heads, n, 32, seed=ws, biased=True, uq=b if shared else None)
    if shared:
        assert (R.query_image(6, b) != torch.arange(6) // 2).any()
    first = _window(geo, q, k, v, dout, bias, shared)
    _window_ref(geo, q, k, v, dout, bias, shared).check(first, _record('window_%s/ws%d' % ('global' if shared else 'local', ws)))
    none = _window(geo, q, k, v, dout, bias, shared, 'none')
    _same_bits(dict(first, dbias=None), none, 'dbias == NULL')
    prior = torch.randn(heads, n, n, generator=torch.Generator().manual_seed(5))
    acc = _window(geo, q, k, v, dout, bias, shared, 'add', prior)
    _accumulated(acc['dbias'], prior, first['dbias'])
    _same_bits(dict(first, dbias=None), dict(acc, dbias=None), 'dbias_accumulate')


# ---- adversarial logits ----------------------------------------------------------------------------------------------------------
DENSE_ADV = (2, 2, 193)                 # b, heads, n: three full tiles and one key
WINDOW_ADV = (3, 12, 24, 2, 12)         # N = 144: two tiles and exactly one wave
ADVERSARIAL = [(kind, fam) for kind in R.KINDS if kind != 'random' for fam in ('plain', 'biased', 'local', 'global')
               if not (fam == 'plain' and kind in ('bias_decides', 'tile_masked', 'first_tile_masked', 'row_masked'))]


def _adversarial(kind, fam):
    if fam in ('plain', 'biased'):
        b, heads, n = DENSE_ADV
        q, k, v, dout, bias = R.make(kind, b, heads, n, 64, seed=7, biased=fam == 'biased')
        chunks = R.dbias_chunks(b, n, heads, DENSE_MAX_CHUNKS)[1]
        return (q, k, v, dout, bias), R.Ref(q, k, v, dout, bias, chunks=chunks), _dense(q, k, v, dout, bias, what=kind)
    geo, shared = WINDOW_ADV, fam == 'global'
    q, k, v, dout, bias = R.make(kind, 6, geo[3], geo[4] ** 2, 32, seed=7, biased=True, uq=geo[0] if shared else None)
    return (q, k, v, dout, bias), _window_ref(geo, q, k, v, dout, bias, shared), _window(geo, q, k, v, dout, bias, shared, what=kind)


@pytest.mark.parametrize('kind,fam', ADVERSARIAL, ids=lambda x: str(x))
def test_adversarial_logits(kind, fam):
    (q, k, v, dout, bias), ref, res = _adversarial(kind, fam)
    for t in res.values():
        assert t is None or torch.isfinite(t.float()).all()
    ref.check(res, _record('adversarial_%s/%s' % (fam, kind)))
    n = k.shape[2]
    grads = [res[x] for x in ('dq', 'dq_global', 'dk', 'dv', 'dbias') if res.get(x) is not None]
    if kind == 'uniform':
        # out = mean of V and lse = ln N, to the derived bounds (the reference was shown to be exactly that on the CPU)
        mean_v = v.double().mean(2, keepdim=True).expand_as(ref.out)
        assert ((res['out'].double() - mean_v).abs() <= ref.bound('out') + 1e-12 * mean_v.abs()).all()
        assert ((res['lse'].double() - math.log(n)).abs() <= ref.bound('lse') + 1e-12).all()
    if kind == 'dout_zero':
        for g in grads:
            assert not _bits(g).any(), 'a zero output gradient gives gradients that are exactly zero'
    if kind == 'dout_one_row':
        heads, row = k.shape[1], n // 2
        for name in ('dq', 'dq_global', 'dk', 'dv'):
            if res.get(name) is None:
                continue
            mine, want = res[name].float(), getattr(ref, name)
            assert not mine[:, :heads - 1].any(), f'{name}: another head got a gradient'
            live_mine, live_ref = mine.abs().sum(-1) != 0, want.abs().sum(-1) != 0
            assert torch.equal(live_mine, live_ref), f'{name}: the rows that carry a gradient differ from the reference'
        assert int((ref.dq_global if ref.dq is None else ref.dq).abs().sum(-1).ne(0).sum()) == 1
        if res['dbias'] is not None:
            assert not res['dbias'][:heads - 1].any()
            assert torch.equal(res['dbias'].abs().sum(-1) != 0, ref.dbias.abs().sum(-1) != 0)
            assert (res['dbias'][heads - 1].abs().sum(-1) != 0).nonzero().tolist() == [[row]]


# ---- limits ----------------------------------------------------------------------------------------------------------------------
def test_largest_grid_y_of_the_dense_family():
    """batch * heads == 65535, the largest grid.y admitted, with one token.  The answer is trivial: out = v and dv = dout bit for
    bit (P = 1), lse = s = q.k / 8, dq = dk = 0 as far as dP - delta goes: dP is an MFMA sum and delta an fmaf chain of the same
    64 products, so dS is a few fp32 roundings of sum |dO||v| and not 0; the reference's bound of dq and dk says how few."""
    b, heads, n = 65535, 1, 1
    g = torch.Generator().manual_seed(3)
    q, k, v, dout = (torch.randn(b, heads, n, 64, generator=g).to(BF) for _ in range(4))
    res = _dense(q, k, v, dout)
    assert torch.equal(_bits(res['out']), _bits(v)) and torch.equal(_bits(res['dv']), _bits(dout))
    ref = R.Ref(q, k, v, dout)
    assert float(ref.dq.abs().max()) < 1e-13 and float(ref.dk.abs().max()) < 1e-13
    ref.check({x: res[x] for x in ('out', 'lse', 'dq', 'dk', 'dv')}, _record('limits/units_65535'))
    s = (q.double() * k.double()).sum(-1) * 0.125
    sa = (q.double().abs() * k.double().abs()).sum(-1) * 0.125
    # one logit: the MFMA sum (4 e of sum |q||k|), the two products and the constant of the scale: 8 e in all
    assert ((res['lse'].double() - s).abs() <= 8 * U32 * sa).all()


def test_biased_at_the_largest_token_count_with_dbias():
    """n = TOK_GLOBAL_ATTN_MAX_TOKENS: 64 x 64 tiles of d(bias) in grid.x, the fold over n * n elements"""
    b, heads, n = 1, 1, 4096
    q, k, v, dout, bias = R.make('random', b, heads, n, 64, seed=4096, biased=True)
    assert _C.lib().tok_global_attn_bias_bwd_chunks(b, n, heads) == R.dbias_chunks(b, n, heads, DENSE_MAX_CHUNKS)[1] == 1
    res = _dense(q, k, v, dout, bias)
    ref = R.Ref(q, k, v, dout, bias, chunks=1)
    ref.check(res, _record('limits/biased_n4096'))


def test_dense_chunks_hold_several_images_and_the_last_is_short():
    b, heads, n = 67, 2, 65
    per, chunks = R.dbias_chunks(b, n, heads, DENSE_MAX_CHUNKS)
    assert (per, chunks) == (2, 34) and b - per * (chunks - 1) == 1
    assert _C.lib().tok_global_attn_bias_bwd_chunks(b, n, heads) == chunks
    for shape in ((70, 5, 1), (3, 5, 2), (130, 65, 1), (256, 197, 12), (1, 4096, 1), (64, 4096, 1), (65535, 1, 1)):
        assert _C.lib().tok_global_attn_bias_bwd_chunks(*shape) == R.dbias_chunks(*shape, DENSE_MAX_CHUNKS)[1], shape
    q, k, v, dout, bias = R.make('random', b, heads, n, 64, seed=67, biased=True)
    R.Ref(q, k, v, dout, bias, chunks=chunks).check(_dense(q, k, v, dout, bias), _record('limits/dense_chunks'))


@pytest.mark.parametrize('shared', [False, True], ids=['local', 'global'])
def test_largest_window_with_several_windows_per_chunk(shared):
    """N = 256 (four full tiles, the largest served) and 129 windows: 128 chunks at most, so two windows per chunk, 65 chunks, the
    last holds one"""
    geo = (43, 16, 48, 1, 16)
    b, h, w, heads, ws = geo
    units, n = 129, 256
    per, chunks = _window_chunks(geo)
    assert (per, chunks) == (2, 65) and units - per * (chunks - 1) == 1
    lib = _C.lib()
    partial = lib.tok_gc_attn_bwd_ws_bytes(b, h, w, heads, ws, int(shared), 1) - lib.tok_gc_attn_bwd_ws_bytes(b, h, w, heads, ws,
                                                                                                            int(shared), 0)
    assert partial == chunks * heads * n * n * 4
    q, k, v, dout, bias = R.make('random', units, heads, n, 32, seed=256, biased=True, uq=b if shared else None)
    res = _window(geo, q, k, v, dout, bias, shared)
    _window_ref(geo, q, k, v, dout, bias, shared).check(res, _record('limits/window_n256_%s' % ('global' if shared else 'local')))


# ---- identities between the families ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ws', [1, 9, 12, 16])
def test_global_mode_fed_the_q_columns_is_local_mode(ws):
    geo = (1, ws, ws, 3, ws)                       # B = 1, one window: q_global of the image is the window's q
    q, k, v, dout, bias = R.make('random', 1, 3, ws * ws, 32, seed=30 + ws, biased=True)
    local = _window(geo, q, k, v, dout, bias, False)
    glob = _window(geo, q, k, v, dout, bias, True)
    local['dq_global'] = local.pop('dq')
    _same_bits(local, glob, 'global mode fed the q columns')


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_misaligned_tensors_are_refused_and_nothing_is_written():
    """qkv, out, dout, dqkv, q_global and dq_global are read or mirrored in 16-byte pieces: a base 8 bytes off is refused"""
    lib, st = _C.lib(), stream_ptr()

    def refused(rc, who):
        err = last_error()
        assert rc == ERR_INVALID and who in err and '16-byte aligned' in err, (rc, err)
    # dense
    b, n, heads = 2, 6, 1
    c, ldb = heads * 64, 8
    qkv = torch.zeros(b * n * 3 * c + 8, dtype=BF, device='cuda')
    dout = torch.zeros(b * n * c + 8, dtype=BF, device='cuda')
    bias = torch.zeros(heads * n * ldb, dtype=F32, device='cuda')
    og, dg = G._out(b * n, c + 8), G._out(b * n, 3 * c + 8)
    lg, dbg = G._out(b * heads, n, F32), G._out(heads * n, ldb, F32)
    ws_bytes = lib.tok_global_attn_bias_bwd_ws_bytes(b, n, heads, ldb)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device='cuda')
    P = dict(qkv=qkv.data_ptr(), out=og.ptr, dout=dout.data_ptr(), dqkv=dg.ptr)

    def fwd(biased, **off):
        p = {k_: v_ + 8 * (k_ in off) for k_, v_ in P.items()}
        if biased:
            return lib.tok_global_attn_bias_fwd(p['qkv'], 3 * c, bias.data_ptr(), ldb, b, n, heads, 64, p['out'], c, lg.ptr, st)
        return lib.tok_global_attn_fwd(p['qkv'], 3 * c, b, n, heads, 64, p['out'], c, lg.ptr, st)

    def bwd(biased, **off):
        p = {k_: v_ + 8 * (k_ in off) for k_, v_ in P.items()}
        if biased:
            return lib.tok_global_attn_bias_bwd(p['qkv'], 3 * c, p['out'], p['dout'], c, lg.ptr, bias.data_ptr(), ldb, b, n, heads,
                                                64, p['dqkv'], 3 * c, dbg.ptr, 0, ws.data_ptr(), ws_bytes, st)
        return lib.tok_global_attn_bwd(p['qkv'], 3 * c, p['out'], p['dout'], c, lg.ptr, b, n, heads, 64, p['dqkv'], 3 * c,
                                       ws.data_ptr(), ws_bytes, st)
    for biased in (False, True):
        tag = 'tok_global_attn_bias' if biased else 'tok_global_attn'
        for name in ('qkv', 'out'):
            refused(fwd(biased, **{name: 1}), tag + '_fwd')
        for name in ('qkv', 'out', 'dout', 'dqkv'):
            refused(bwd(biased, **{name: 1}), tag + '_bwd')
    # windowed
    wb, h, w, wh, wsz = 2, 4, 8, 1, 4
    wc, wn, total = 32, 16, 2 * 4 * 8
    kv = torch.zeros(total * 3 * wc + 8, dtype=BF, device='cuda')
    qgl = torch.zeros(wb * wn * wc + 8, dtype=BF, device='cuda')
    wdo = torch.zeros(total * wc + 8, dtype=BF, device='cuda')
    wbias = torch.zeros(wh * wn * wn, dtype=F32, device='cuda')
    wo, wd, wdq = G._out(total, wc + 8), G._out(total, 3 * wc + 8), G._out(wb * wn, wc + 8)
    wl, wdb = G._out(wb * 2 * wh, wn, F32), G._out(wh * wn, wn, F32)
    WP = dict(qkv=kv.data_ptr(), q_global=qgl.data_ptr(), out=wo.ptr, dout=wdo.data_ptr(), dqkv=wd.ptr, dq_global=wdq.ptr)

    def gc(back, shared, **off):
        p = {k_: v_ + 8 * (k_ in off) for k_, v_ in WP.items()}
        ld = (2 if shared else 3) * wc
        qp, dqp = (p['q_global'], p['dq_global']) if shared else (None, None)
        if not back:
            return lib.tok_gc_attn_fwd(p['qkv'], ld, qp, wc, wbias.data_ptr(), wn, wb, h, w, wc, wh, wsz, p['out'], wc, wl.ptr, st)
        nbytes = lib.tok_gc_attn_bwd_ws_bytes(wb, h, w, wh, wsz, int(shared), 1)
        buf = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')
        return lib.tok_gc_attn_bwd(p['qkv'], ld, qp, wc, wbias.data_ptr(), wn, p['out'], p['dout'], wc, wl.ptr, wb, h, w, wc, wh, wsz,
                                   p['dqkv'], ld, dqp, wc, wdb.ptr, 0, buf.data_ptr(), nbytes, st)
    for shared in (False, True):
        for name in ('qkv', 'out') + (('q_global',) if shared else ()):
            refused(gc(False, shared, **{name: 1}), 'tok_gc_attn_fwd')
        for name in ('qkv', 'out', 'dout', 'dqkv') + (('q_global', 'dq_global') if shared else ()):
            refused(gc(True, shared, **{name: 1}), 'tok_gc_attn_bwd')
    torch.cuda.synchronize()
    for t in (og, dg, lg, dbg, wo, wd, wdq, wl, wdb):
        t.check('refused call')
        assert t.untouched(), 'a refused call wrote an output'
