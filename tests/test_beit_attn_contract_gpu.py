"""The kernels BEiT adds, against fp64 and across the contract of include/tok.h: global attention with an additive bias and its
d(bias) (csrc/attn_global.hip), the relative-position gather and its transpose (csrc/transformer.hip), the LayerScale residual
(csrc/layer_scale.hip).  Guarded buffers (tests/helpers.py), NaN input pads (the bias rows included), every element checked.

Bounds.  out / lse / dq / dk / dv: those of tests/test_global_attn_contract_gpu.py, restated in beit_ref.check_attention.
dbias: |dbias - ref| <= 2^-7 M + 2^-24 max M with M[h,i,j] = sum_b P (|dO| |V|^T + sum_d |dO| |O|): O is stored in bf16 before
delta (2^-9) and dS may be rounded to bf16 once (2^-9), together 2^-8 M, doubled for margin as the forward bound is."""
import pytest
import torch

import beit_ref as R
from helpers import Guarded, assert_bounded, record_distance
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
BF, F32, I64 = torch.bfloat16, torch.float32, torch.int64
HD = 64
U32 = 2.0 ** -24


def _nan_rows(values, rows, cols, ld):
    """fp32 input [rows][cols] inside a [rows + 1][ld] buffer whose pad columns and guard row hold NaN"""
    buf = torch.full((rows + 1, ld), float('nan'), dtype=F32, device='cuda')
    buf[:rows, :cols] = values.reshape(rows, cols)
    return buf


def _ldb(n):
    return (n + 3) // 4 * 4 + 4


def _launch(qkv, bias, b, n, heads, dout, dbias_init=None, want_dbias=True):
    lib, st = _C.lib(), stream_ptr()
    c = heads * HD
    ldq, ldo, ldd, ldb = 3 * c + 8, c + 24, 3 * c + 16, _ldb(n)
    qg = Guarded(b * n, 3 * c, ldq, init=qkv.cuda(), nan_pad=True)
    bg = _nan_rows(bias.cuda(), heads * n, n, ldb)
    og = Guarded(b * n, c, ldo)
    lg = Guarded(b * heads, n, dtype=F32)
    _C.check(lib.tok_global_attn_bias_fwd(qg.ptr, ldq, bg.data_ptr(), ldb, b, n, heads, HD, og.ptr, ldo, lg.ptr, st), 'fwd')
    gg = Guarded(b * n, c, ldo, init=dout.cuda(), nan_pad=True)
    dg = Guarded(b * n, 3 * c, ldd)
    dbg = Guarded(heads * n, n, ldb, dtype=F32, init=None if dbias_init is None else dbias_init.cuda())
    ws_bytes = lib.tok_global_attn_bias_bwd_ws_bytes(b, n, heads, ldb)
    wsg = Guarded(1, ws_bytes // 4, dtype=F32)
    _C.check(lib.tok_global_attn_bias_bwd(qg.ptr, ldq, og.ptr, gg.ptr, ldo, lg.ptr, bg.data_ptr(), ldb, b, n, heads, HD, dg.ptr,
                                          ldd, dbg.ptr if want_dbias else None, 0 if dbias_init is None else 1, wsg.ptr,
                                          ws_bytes, st), 'bwd')
    torch.cuda.synchronize()
    for buf, what in ((qg, 'qkv'), (og, 'out'), (lg, 'lse'), (gg, 'dout'), (dg, 'dqkv'), (wsg, 'ws'), (dbg, 'dbias')):
        buf.check(what)
    assert torch.isnan(bg[:heads * n, n:]).all() and torch.isnan(bg[heads * n]).all()
    return og.value(), lg.value(), dg.value(), dbg.value().view(heads, n, n)


def _inputs(b, n, heads, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(b * n, 3 * heads * HD, generator=g) * 1.5).to(BF)
    dout = torch.randn(b * n, heads * HD, generator=g).to(BF)
    bias = torch.randn(heads, n, n, generator=g) * 2                 # N(0, 2^2): it moves the softmax
    return qkv, dout, bias


# (batch, n, heads): smallest; 2x2 grid; exactly one tile; one key and one query past the tile; the real layer; 384 px; and a
# batch larger than the d(bias) chunk count can cover with one image each (64 chunks at most), so chunks hold two images; the
# same with 2 x 2 tiles that have a tail in both directions, three images per chunk and a last chunk of one image
SHAPES = [(1, 2, 1), (3, 5, 2), (2, 64, 1), (2, 65, 2), (4, 197, 12), (1, 577, 1), (70, 5, 1), (130, 65, 1)]
_cache = {}


def _case(shape):
    """inputs, fp64 reference and the kernel's results of a shape: computed once, shared, never modified"""
    if shape not in _cache:
        b, n, heads = shape
        qkv, dout, bias = _inputs(b, n, heads, seed=1000 * b + n + heads)
        _cache[shape] = (qkv, dout, bias, R.AttnRef(qkv, bias, b, n, heads, dout), _launch(qkv, bias, b, n, heads, dout))
    return _cache[shape]


def test_the_chunk_fold_runs():
    lib = _C.lib()
    assert lib.tok_global_attn_bias_bwd_chunks(70, 5, 1) == 35          # two images per chunk, 35 partials folded
    assert lib.tok_global_attn_bias_bwd_chunks(3, 5, 2) == 3
    assert lib.tok_global_attn_bias_bwd_chunks(130, 65, 1) == 44        # 4 tiles: 64 chunks wanted, 3 images each, the last holds 1
    assert lib.tok_global_attn_bias_bwd_chunks(256, 197, 12) == 11      # 192 tiles x 11 chunks = 2112 workgroups


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'b%d_n%d_h%d' % s)
def test_biased_attention_against_fp64(shape):
    b, n, heads = shape
    qkv, dout, bias, ref, (out, lse, dqkv, dbias) = _case(shape)
    tag = 'beit_attn_contract/b%d_n%d_h%d' % shape
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv.float()).all()
    assert torch.isfinite(dbias).all()

    def record(worst):
        print(tag, {k: round(v, 4) for k, v in worst.items()})
        for k, v in worst.items():
            record_distance(tag, k, err_over_bound=v)
    R.check_attention(ref, out, lse, dqkv, dbias, heads, record=record)


@pytest.mark.parametrize('shape', [(3, 5, 2), (2, 65, 2), (70, 5, 1)], ids=lambda s: 'b%d_n%d_h%d' % s)
def test_two_runs_give_the_same_bits_and_accumulate_adds(shape):
    b, n, heads = shape
    qkv, dout, bias, ref, first = _case(shape)
    again = _launch(qkv, bias, b, n, heads, dout)
    for x, y in zip(first, again):
        assert torch.equal(x.view(torch.int16 if x.dtype == BF else torch.int32), y.view(torch.int16 if y.dtype == BF else torch.int32))
    prior = torch.randn(heads, n, n, generator=torch.Generator().manual_seed(5))
    acc = _launch(qkv, bias, b, n, heads, dout, dbias_init=prior)[3]
    want = prior.double() + first[3].double()
    assert ((acc.double() - want).abs() <= U32 * want.abs() + 1e-45).all()       # one fp32 rounding of the sum
    # dbias == NULL: dq / dk / dv alone, same bits
    none = _launch(qkv, bias, b, n, heads, dout, want_dbias=False)
    assert torch.equal(none[2].view(torch.int16), first[2].view(torch.int16))


@pytest.mark.parametrize('shape', [(1, 2, 1), (2, 65, 2), (4, 197, 12)], ids=lambda s: 'b%d_n%d_h%d' % s)
def test_zero_bias_gives_the_bits_of_the_unbiased_kernels(shape):
    b, n, heads = shape
    lib, st = _C.lib(), stream_ptr()
    c = heads * HD
    qkv, dout, _ = _inputs(b, n, heads, seed=77 + n)
    out, lse, dqkv, _ = _launch(qkv, torch.zeros(heads, n, n), b, n, heads, dout)
    q, g = qkv.cuda(), dout.cuda()
    o0 = torch.empty(b * n, c, dtype=BF, device='cuda')
    l0 = torch.empty(b * heads, n, dtype=F32, device='cuda')
    d0 = torch.empty(b * n, 3 * c, dtype=BF, device='cuda')
    _C.check(lib.tok_global_attn_fwd(q.data_ptr(), 3 * c, b, n, heads, HD, o0.data_ptr(), c, l0.data_ptr(), st), 'fwd')
    ws_bytes = lib.tok_global_attn_bwd_ws_bytes(b, n, heads)
    ws = torch.empty(ws_bytes // 4, dtype=F32, device='cuda')
    _C.check(lib.tok_global_attn_bwd(q.data_ptr(), 3 * c, o0.data_ptr(), g.data_ptr(), c, l0.data_ptr(), b, n, heads, HD,
                                     d0.data_ptr(), 3 * c, ws.data_ptr(), ws_bytes, st), 'bwd')
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), o0.cpu().view(torch.int16))
    assert torch.equal(lse.view(torch.int32), l0.cpu().view(torch.int32))
    assert torch.equal(dqkv.view(torch.int16), d0.cpu().view(torch.int16))


# ---- relative-position gather and its transpose --------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', [(1, 1), (2, 2), (14, 14), (7, 3)], ids=lambda g: '%dx%d' % g)
def test_relpos_gather_and_transpose(grid):
    lib, st = _C.lib(), stream_ptr()
    heads = 3
    index = R.gen_relative_position_index(grid)
    n, rows = index.shape[0], int(index.max()) + 1
    ldb = _ldb(n)
    g = torch.Generator().manual_seed(n)
    table = torch.randn(rows, heads, generator=g)
    bg = Guarded(heads * n, n, ldb, dtype=F32)
    idx = index.cuda()
    _C.check(lib.tok_relpos_bias_fwd(table.cuda().data_ptr(), idx.data_ptr(), heads, n, bg.ptr, ldb, st), 'relpos fwd')
    torch.cuda.synchronize()
    bg.check('bias')
    assert torch.equal(bg.value().view(heads, n, n), R.relpos_bias(table, index))          # exact
    count = torch.bincount(index.reshape(-1), minlength=rows).double()

    def transpose(dbias, prior=None):
        dg = _nan_rows(dbias.cuda(), heads * n, n, ldb)
        tg = Guarded(rows, heads, dtype=F32, init=None if prior is None else prior.cuda())
        _C.check(lib.tok_relpos_bias_bwd(dg.data_ptr(), ldb, idx.data_ptr(), heads, n, rows, tg.ptr, 0 if prior is None else 1,
                                         st), 'relpos bwd')
        torch.cuda.synchronize()
        tg.check('dtable')
        return tg.value()

    def ref_of(dbias):
        flat = dbias.double().permute(1, 2, 0).reshape(n * n, heads)
        return torch.zeros(rows, heads, dtype=torch.float64).index_add_(0, index.reshape(-1), flat)
    ints = torch.randint(-8, 9, (heads, n, n), generator=g).float()
    assert torch.equal(transpose(ints).double(), ref_of(ints))                             # small integers: bit-exact
    prior = torch.randint(-8, 9, (rows, heads), generator=g).float()
    assert torch.equal(transpose(ints, prior).double(), ref_of(ints) + prior.double())
    reals = torch.randn(heads, n, n, generator=g)
    bound = count[:, None] * U32 * ref_of(reals.abs())
    assert ((transpose(reals).double() - ref_of(reals)).abs() <= bound).all()
    assert torch.equal(transpose(reals), transpose(reals))


def test_relpos_gather_past_one_trip_of_the_capped_grid():
    """heads * n * n > 2^24 = 65536 blocks x 256 threads, the most one trip of the gather's capped grid covers (16 heads x 1025^2
    of beit_large_patch16_512 is such a size): every element is written, none outside.  The C-ABI takes any index into the
    table, so a drawn one over a short table keeps the transpose (one block per table row) quick."""
    lib, st = _C.lib(), stream_ptr()
    heads, n, rows = 4, 2049, 61
    assert heads * n * n > 2 ** 24
    ldb = _ldb(n)
    g = torch.Generator().manual_seed(9)
    table = torch.randn(rows, heads, generator=g).cuda()
    idx = torch.randint(0, rows, (n, n), generator=g).cuda()
    bg = Guarded(heads * n, n, ldb, dtype=F32)
    _C.check(lib.tok_relpos_bias_fwd(table.data_ptr(), idx.data_ptr(), heads, n, bg.ptr, ldb, st), 'relpos fwd')
    torch.cuda.synchronize()
    bg.check('bias')
    assert torch.equal(bg.view.reshape(heads, n, n), table[idx.view(-1)].view(n, n, heads).permute(2, 0, 1))      # exact
    ints = torch.randint(-8, 9, (heads, n, n), generator=g).float().cuda()
    dg = torch.full((heads * n + 1, ldb), float('nan'), dtype=F32, device='cuda')
    dg[:heads * n, :n] = ints.view(heads * n, n)
    tg = Guarded(rows, heads, dtype=F32)
    _C.check(lib.tok_relpos_bias_bwd(dg.data_ptr(), ldb, idx.data_ptr(), heads, n, rows, tg.ptr, 0, st), 'relpos bwd')
    torch.cuda.synchronize()
    tg.check('dtable')
    want = torch.zeros(rows, heads, dtype=torch.float64, device='cuda').index_add_(
        0, idx.view(-1), ints.double().permute(1, 2, 0).reshape(n * n, heads))
    assert torch.equal(tg.view.double(), want)            # small integers (|sum| < 2^24): bit-exact


def test_relpos_gather_of_beit_large_512_takes_a_second_trip():
    """16 heads on a 32 x 32 grid (n = 1025, beit_large_patch16_512), the case relpos_bias_fwd_kernel's comment names: 16 * 1025^2 is
    just past the 2^24 elements one trip of the capped grid covers.  With the model's own index; exact."""
    lib, st = _C.lib(), stream_ptr()
    heads = 16
    index = R.gen_relative_position_index((32, 32))
    n, rows = index.shape[0], int(index.max()) + 1
    assert n == 1025 and 2 ** 24 < heads * n * n < 2 ** 24 + 2 ** 16
    ldb = _ldb(n)
    table = torch.randn(rows, heads, generator=torch.Generator().manual_seed(5)).cuda()
    idx = index.cuda()
    bg = Guarded(heads * n, n, ldb, dtype=F32)
    _C.check(lib.tok_relpos_bias_fwd(table.data_ptr(), idx.data_ptr(), heads, n, bg.ptr, ldb, st), 'relpos fwd')
    torch.cuda.synchronize()
    bg.check('bias')
    want = table[idx.view(-1)].view(n, n, heads).permute(2, 0, 1)
    assert torch.equal(bg.view.reshape(heads, n, n).view(torch.int32), want.contiguous().view(torch.int32))      # exact


# ---- LayerScale residual ---------------------------------------------------------------------------------------------------------
def _layer_scale(x, a, gamma, scale, rps, dout, da_prior=None, dg_prior=None):
    lib, st = _C.lib(), stream_ptr()
    rows, d = x.shape
    xg = Guarded(rows, d, init=x.cuda(), nan_pad=True)
    ag = Guarded(rows, d, init=a.cuda(), nan_pad=True)
    og = Guarded(rows, d)
    gm = gamma.cuda()
    sc = None if scale is None else scale.cuda()
    sp = None if sc is None else sc.data_ptr()
    _C.check(lib.tok_layer_scale_fwd(xg.ptr, ag.ptr, gm.data_ptr(), sp, rps, og.ptr, rows, d, st), 'layer_scale fwd')
    gg = Guarded(rows, d, init=dout.cuda(), nan_pad=True)
    dag = Guarded(rows, d, init=None if da_prior is None else da_prior.cuda())
    dgg = Guarded(1, d, dtype=F32, init=None if dg_prior is None else dg_prior.cuda())
    nrows = lib.tok_layer_scale_bwd_rows(rows, d)
    pg = Guarded(nrows, d, dtype=F32)
    _C.check(lib.tok_layer_scale_bwd(gg.ptr, ag.ptr, gm.data_ptr(), sp, rps, dag.ptr, 0 if da_prior is None else 1, dgg.ptr,
                                     0 if dg_prior is None else 1, pg.ptr, rows, d, st), 'layer_scale bwd')
    torch.cuda.synchronize()
    for buf, what in ((og, 'out'), (dag, 'da'), (dgg, 'dgamma'), (pg, 'partial')):
        buf.check(what)
    return og.value(), dag.value(), dgg.value().view(d), nrows


def _ls_ref(x, a, gamma, scale, rps, dout):
    rows = x.shape[0]
    s = torch.ones(rows, 1, dtype=torch.float64) if scale is None else scale.double().repeat_interleave(rps)[:, None]
    xd, ad, gd, dd = x.double(), a.double(), gamma.double()[None], dout.double()
    return xd + s * gd * ad, s * gd * dd, (s * dd * ad).sum(0), s


# (rows, d, rows per sample): one row; 5 tokens x 3 images; the real layer at B = 2; more rows than the 512-block cap covers in
# one trip at d = 8 (256 rows per block); d > 2048: two channel-group passes per lane, the second one ragged
LS_SHAPES = [(1, 8, 1), (15, 128, 5), (394, 768, 197), (512 * 256 + 37 * 3 - 512 * 256 % 3, 8, 3), (36, 2176, 12)]


@pytest.mark.parametrize('rows,d,rps', LS_SHAPES, ids=lambda v: str(v))
def test_layer_scale(rows, d, rps):
    assert rows % rps == 0
    g = torch.Generator().manual_seed(rows + d)
    # small integers, dyadic gamma, scales in {0, 1, 2}: every result is exact in bf16 / fp32, so bit for bit
    x = torch.randint(-8, 9, (rows, d), generator=g).to(BF)
    a = torch.randint(-4, 5, (rows, d), generator=g).to(BF)
    dout = torch.randint(-4, 5, (rows, d), generator=g).to(BF)
    gamma = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (d,), generator=g)]
    scale = torch.randint(0, 3, (rows // rps,), generator=g).float()
    out, da, dgam, nrows = _layer_scale(x, a, gamma, scale, rps, dout)
    r_out, r_da, r_dg, _ = _ls_ref(x, a, gamma, scale, rps, dout)
    assert torch.equal(out.double(), r_out) and torch.equal(da.double(), r_da) and torch.equal(dgam.double(), r_dg)
    if rows > 512 * 256:
        assert nrows == 512
    prior_a = torch.randint(-4, 5, (rows, d), generator=g).to(BF)
    prior_g = torch.randint(-4, 5, (d,), generator=g).float()
    _, da2, dg2, _ = _layer_scale(x, a, gamma, scale, rps, dout, prior_a, prior_g)
    assert torch.equal(da2.double(), r_da + prior_a.double()) and torch.equal(dg2.double(), r_dg + prior_g.double())
    # reals, with and without the drop-path scales
    x, a, dout = (torch.randn(rows, d, generator=g).to(BF) for _ in range(3))
    gamma = 0.1 + 0.05 * torch.randn(d, generator=g)
    for sc in (None, torch.tensor([0.0, 1.0 / 0.9])[torch.randint(0, 2, (rows // rps,), generator=g)]):
        out, da, dgam, _ = _layer_scale(x, a, gamma, sc, rps, dout)
        r_out, r_da, r_dg, s = _ls_ref(x, a, gamma, sc, rps, dout)
        ga = (s * gamma.double()[None] * a.double()).abs()
        assert_bounded(out, r_out, x.double().abs() + ga, 2.0 ** -8, 4 * U32, 'layer_scale out')
        assert_bounded(da, r_da, (s * gamma.double()[None] * dout.double()).abs(), 2.0 ** -8, 4 * U32, 'layer_scale da')
        assert_bounded(dgam, r_dg, (s * dout.double() * a.double()).abs().sum(0), 0.0, rows * U32, 'layer_scale dgamma')
        again = _layer_scale(x, a, gamma, sc, rps, dout)
        assert torch.equal(again[2], dgam) and torch.equal(again[1].view(torch.int16), da.view(torch.int16))


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _refused(rc, msg):
    err = _C.lib().tok_last_error()
    err = err.decode() if isinstance(err, bytes) else err
    assert rc == -1, (rc, err)
    assert msg in err, (msg, err)


def test_refusals_leave_outputs_untouched():
    lib, st = _C.lib(), stream_ptr()
    b, n, heads = 2, 6, 1
    c = heads * HD
    ldb = 8
    qkv = torch.zeros(b * n, 3 * c, dtype=BF, device='cuda')
    bias = torch.zeros(heads * n * ldb + 4, dtype=F32, device='cuda')
    outs = [Guarded(b * n, c), Guarded(b * heads, n, dtype=F32), Guarded(b * n, 3 * c), Guarded(heads * n, ldb, dtype=F32)]
    og, lg, dg, dbg = outs
    ws_bytes = lib.tok_global_attn_bias_bwd_ws_bytes(b, n, heads, ldb)
    ws = torch.zeros(ws_bytes // 4, dtype=F32, device='cuda')

    def fwd(bias_ptr=bias.data_ptr(), ld=ldb, hd=HD, qp=qkv.data_ptr()):
        return lib.tok_global_attn_bias_fwd(qp, 3 * c, bias_ptr, ld, b, n, heads, hd, og.ptr, c, lg.ptr, st)

    def bwd(bias_ptr=bias.data_ptr(), ld=ldb, ldd=3 * c, wsb=ws_bytes):
        return lib.tok_global_attn_bias_bwd(qkv.data_ptr(), 3 * c, og.ptr, og.ptr, c, lg.ptr, bias_ptr, ld, b, n, heads, HD,
                                            dg.ptr, ldd, dbg.ptr, 0, ws.data_ptr(), wsb, st)
    _refused(fwd(bias_ptr=None), 'bias')
    _refused(fwd(ld=4), 'ldb')                       # ldb < n
    _refused(fwd(ld=7), 'ldb')                       # not a multiple of 4
    _refused(fwd(bias_ptr=bias.data_ptr() + 4), 'bias')      # not 16-byte aligned
    _refused(fwd(hd=32), 'head_dim')
    _refused(fwd(qp=None), 'null')
    _refused(bwd(bias_ptr=None), 'bias')
    _refused(bwd(ld=6), 'ldb')
    _refused(bwd(ldd=3 * c - 8), 'ldd')
    assert bwd(wsb=ws_bytes - 1) == -3
    assert lib.tok_global_attn_bias_bwd_ws_bytes(b, n, heads, 4) == 0
    # relative-position bias
    idx = torch.zeros(n * n, dtype=I64, device='cuda')
    tab = torch.zeros(4 * 40, dtype=F32, device='cuda')
    bo = Guarded(heads * n, ldb, dtype=F32)
    to = Guarded(4, 40, dtype=F32)
    _refused(lib.tok_relpos_bias_fwd(None, idx.data_ptr(), heads, n, bo.ptr, ldb, st), 'relpos')
    _refused(lib.tok_relpos_bias_fwd(tab.data_ptr(), idx.data_ptr(), heads, n, bo.ptr, n - 1, st), 'relpos')
    _refused(lib.tok_relpos_bias_fwd(tab.data_ptr(), idx.data_ptr(), 0, n, bo.ptr, ldb, st), 'relpos')
    _refused(lib.tok_relpos_bias_bwd(bias.data_ptr(), ldb, idx.data_ptr(), 33, n, 4, to.ptr, 0, st), 'heads')
    _refused(lib.tok_relpos_bias_bwd(bias.data_ptr(), ldb, None, heads, n, 4, to.ptr, 0, st), 'relpos')
    _refused(lib.tok_relpos_bias_bwd(bias.data_ptr(), ldb, idx.data_ptr(), heads, n, 0, to.ptr, 0, st), 'relpos')
    # LayerScale
    rows, d = 4, 16
    x = torch.zeros(rows, d, dtype=BF, device='cuda')
    gam = torch.zeros(d, dtype=F32, device='cuda')
    lo, la, lgm, lp = Guarded(rows, d), Guarded(rows, d), Guarded(1, d, dtype=F32), Guarded(4, d, dtype=F32)
    _refused(lib.tok_layer_scale_fwd(x.data_ptr(), x.data_ptr(), gam.data_ptr(), None, 0, lo.ptr, rows, 12, st), 'sizes')
    _refused(lib.tok_layer_scale_fwd(x.data_ptr(), x.data_ptr(), None, None, 0, lo.ptr, rows, d, st), 'null')
    _refused(lib.tok_layer_scale_fwd(x.data_ptr(), x.data_ptr(), gam.data_ptr(), gam.data_ptr(), 0, lo.ptr, rows, d, st), 'sizes')
    _refused(lib.tok_layer_scale_fwd(x.data_ptr(), x.data_ptr(), gam.data_ptr(), None, 0, lo.ptr, 0, d, st), 'sizes')
    _refused(lib.tok_layer_scale_bwd(x.data_ptr(), x.data_ptr(), gam.data_ptr(), None, 0, la.ptr, 0, lgm.ptr, 0, None, rows, d, st),
             'null')
    _refused(lib.tok_layer_scale_bwd(x.data_ptr(), x.data_ptr(), gam.data_ptr(), None, 0, la.ptr, 0, lgm.ptr, 0, lp.ptr, rows, 20,
                                     st), 'sizes')
    assert lib.tok_layer_scale_bwd_rows(rows, 12) == 0
    torch.cuda.synchronize()
    for t in outs + [bo, to, lo, la, lgm, lp]:
        t.check('refused call')
        iv = t.view.view(torch.int16 if t.dtype == BF else torch.int32)
        assert (iv == t.bits).all(), 'a refused call wrote an output'


def test_engine_refuses_an_index_outside_the_table():
    from torchok_amd import engine
    from torchok_amd.engine import transformer as ET
    table = torch.nn.Parameter(torch.zeros(12, 2, device='cuda'))
    index = R.gen_relative_position_index((2, 2)).cuda()
    with torch.no_grad(), engine.region() as r:
        bias, _ = ET.relpos_bias(r, table, index, 2, 5)
        assert tuple(bias.shape[:2]) == (2, 5)
        bad = index.clone()
        bad[3, 2] = 12
        with pytest.raises(ValueError):
            ET.relpos_bias(r, table, bad, 2, 5)
        bad[3, 2] = -1
        with pytest.raises(ValueError):
            ET.relpos_bias(r, table, bad, 2, 5)
