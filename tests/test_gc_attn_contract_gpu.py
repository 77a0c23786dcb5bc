"""The kernels GCViT adds, against fp64 and across the contract of include/tok.h: biased window attention with an optional
shared query and its three gradients (csrc/gc_attn.hip), squeeze-excite with GELU inside and no biases (csrc/se.hip).
Every operand sits in a helpers.GuardedSpan: inputs with NaN in both guards and in their pad columns, outputs and the workspace
prefilled with NaN, guards checked after every call, every element compared.

Bounds: gcvit_ref.check_attention (those of tests/test_beit_attn_contract_gpu.py, derived from the number formats there).

Shapes, each the smallest at which its failure can show:
  a  B 3, 14 x 21, ws 7, 2 heads   nW = 2 x 3 on a non-square map (an h / w transposition), B and nW coprime (u div nW for
                                   u mod B), N = 49 has masked keys
  b  B 2, 28 x 14, ws 14, 1 head   N = 196: four key tiles with a 4-key tail, two windows per image
  c  B 1, 8 x 8, ws 8, 3 heads     N = 64: no masked key, a mask that eats the last real key shows
  d  B 2, 8 x 4, ws 4, 1 head      N = 16: a single partial tile"""
import pytest
import torch

import gcvit_ref as R
from helpers import ERR_INVALID, GuardedSpan, NAN_BITS, assert_bounded, last_error, record_distance
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
HD = 32
U32 = 2.0 ** -24
GUARD = 4096

CASES = {'a': (3, 14, 21, 2, 7), 'b': (2, 28, 14, 1, 14), 'c': (1, 8, 8, 3, 8), 'd': (2, 8, 4, 1, 4)}


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _pitched(values, ld):
    """[rows][cols] values inside NaN rows of pitch ld"""
    rows, cols = values.shape
    buf = torch.full((rows, ld), float('nan'), dtype=values.dtype)
    buf[:, :cols] = values
    return buf


def _in(values, ld):
    t = _pitched(values, ld)
    return GuardedSpan(t.numel(), t.dtype, GUARD, init=t.cuda(), nan_guard=True)


def _out(rows, ld, dtype=BF, init=None):
    """an output of `rows` rows of pitch ld: the NaN fill everywhere (operand, pad columns and guards); `init` [rows][cols]
    fills the leading columns of the rows"""
    span = GuardedSpan(rows * ld, dtype, GUARD, nan_guard=True)
    if init is not None:
        span.view.view(rows, ld)[:, :init.shape[1]] = init.cuda()
    return span


def _value(span, rows, ld, cols):
    """(values [rows][cols], True when every pad column still holds the NaN fill)"""
    v = span.value().view(rows, ld)
    pads = _bits(v[:, cols:])
    return v[:, :cols].contiguous(), bool((pads == NAN_BITS[span.dtype]).all()) if pads.numel() else True


def _launch(geo, qkv, qg, bias, dout, dbias_mode='set', dbias_prior=None):
    """forward + backward with every pitch larger than its width.  dbias_mode: 'set' | 'add' (onto dbias_prior) | 'none'.
    -> out, lse, dqkv, dq_global (None in local mode), dbias (None with 'none')"""
    lib, st = _C.lib(), stream_ptr()
    b, h, w, heads, ws = geo
    c, n, total = heads * HD, ws * ws, b * h * w
    nw = (h // ws) * (w // ws)
    parts = 3 if qg is None else 2
    ld, ldg, ldo, ldd, lddg, ldb = parts * c + 8, c + 16, c + 24, parts * c + 16, c + 8, (n + 3) // 4 * 4 + 4
    xq = _in(qkv, ld)
    xg = None if qg is None else _in(qg, ldg)
    xb = _in(bias.reshape(heads * n, n), ldb)
    og, lg = _out(total, ldo), _out(b * nw * heads, n, F32)
    gp = None if xg is None else xg.ptr
    _C.check(lib.tok_gc_attn_fwd(xq.ptr, ld, gp, ldg, xb.ptr, ldb, b, h, w, c, heads, ws, og.ptr, ldo, lg.ptr, st), 'fwd')
    xd = _in(dout, ldo)
    dg = _out(total, ldd)
    dgg = None if qg is None else _out(b * n, lddg)
    prior = None if dbias_mode != 'add' else dbias_prior.reshape(heads * n, n)
    dbg = _out(heads * n, ldb, F32, init=prior)
    want = dbias_mode != 'none'
    ws_bytes = lib.tok_gc_attn_bwd_ws_bytes(b, h, w, heads, ws, int(qg is not None), int(want))
    wsg = GuardedSpan(ws_bytes, torch.uint8, GUARD, nan_guard=True)
    _C.check(lib.tok_gc_attn_bwd(xq.ptr, ld, gp, ldg, xb.ptr, ldb, og.ptr, xd.ptr, ldo, lg.ptr, b, h, w, c, heads, ws, dg.ptr, ldd,
                                 None if dgg is None else dgg.ptr, lddg, dbg.ptr if want else None, int(dbias_mode == 'add'),
                                 wsg.ptr, ws_bytes, st), 'bwd')
    torch.cuda.synchronize()
    for buf, what in ((xq, 'qkv'), (xg, 'q_global'), (xb, 'bias'), (og, 'out'), (lg, 'lse'), (xd, 'dout'), (dg, 'dqkv'),
                      (dgg, 'dq_global'), (dbg, 'dbias'), (wsg, 'ws')):
        if buf is not None:
            buf.check(what)
    out, ok1 = _value(og, total, ldo, c)
    lse = lg.value().view(b * nw, heads, n)
    dqkv, ok2 = _value(dg, total, ldd, parts * c)
    dqg, ok3 = (None, True) if dgg is None else _value(dgg, b * n, lddg, c)
    dbias, ok4 = _value(dbg, heads * n, ldb, n)
    assert ok1 and ok2 and ok3, 'pad columns of out / d(qkv) / d(q_global) were written'
    if dbias_mode == 'none':
        assert dbg.untouched(), 'a NULL dbias was written'
        dbias = None
    else:
        assert ok4, 'pad columns of dbias were written'
        dbias = dbias.view(heads, n, n)
    return out, lse, dqkv, dqg, dbias


_cache = {}


def _case(name, global_mode):
    """inputs, fp64 reference and the kernel's results of a case: computed once, shared, never modified"""
    key = (name, global_mode)
    if key not in _cache:
        geo = CASES[name]
        qkv, qg, dout, bias = R.attn_inputs(geo, global_mode, seed=100 * ord(name) + global_mode)
        _cache[key] = (qkv, qg, dout, bias, R.AttnRef(qkv, qg, bias, geo, dout), _launch(geo, qkv, qg, bias, dout))
    return _cache[key]


MODES = [pytest.param(False, id='local'), pytest.param(True, id='global')]


@pytest.mark.parametrize('global_mode', MODES)
@pytest.mark.parametrize('name', list(CASES))
def test_attention_against_fp64(name, global_mode):
    geo = CASES[name]
    qkv, qg, dout, bias, ref, (out, lse, dqkv, dqg, dbias) = _case(name, global_mode)
    tag = 'gc_attn_contract/%s_%s' % (name, 'global' if global_mode else 'local')
    for t in (out, lse, dqkv, dqg, dbias):
        assert t is None or torch.isfinite(t.float()).all()          # every element of every output was written

    def record(worst):
        print(tag, {k: round(v, 4) for k, v in worst.items()})
        for k, v in worst.items():
            record_distance(tag, k, err_over_bound=v)
    R.check_attention(ref, out, lse, dqkv, dqg, dbias, geo[3], record=record)


@pytest.mark.parametrize('global_mode', MODES)
@pytest.mark.parametrize('name', list(CASES))
def test_two_runs_give_the_same_bits_and_dbias_modes(name, global_mode):
    geo = CASES[name]
    heads, n = geo[3], geo[4] ** 2
    qkv, qg, dout, bias, ref, first = _case(name, global_mode)
    again = _launch(geo, qkv, qg, bias, dout)
    for x, y in zip(first, again):
        assert (x is None and y is None) or torch.equal(_bits(x), _bits(y))
    prior = torch.randn(heads, n, n, generator=torch.Generator().manual_seed(5))
    acc = _launch(geo, qkv, qg, bias, dout, 'add', prior)[4]
    want = prior.double() + first[4].double()
    assert ((acc.double() - want).abs() <= U32 * want.abs() + 1e-45).all()       # one fp32 rounding of the sum
    none = _launch(geo, qkv, qg, bias, dout, 'none')
    assert none[4] is None
    for x, y in zip(first[:4], none[:4]):
        assert (x is None and y is None) or torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize('global_mode', MODES)
@pytest.mark.parametrize('name', ['a', 'b'])
def test_a_window_depends_on_its_own_tokens_only(name, global_mode):
    geo = CASES[name]
    b, h, w, heads, ws = geo
    qkv, qg, dout, bias, ref, first = _case(name, global_mode)
    idx = R.window_index(b, h, w, ws)
    u = idx.shape[0] - 2
    other = qkv.clone()
    other[idx[u]] = (other[idx[u]].float() * -0.5 + 0.25).to(BF)
    out, lse = _launch(geo, other, qg, bias, dout)[:2]
    rest = torch.ones(idx.shape[0], dtype=torch.bool)
    rest[u] = False
    assert torch.equal(_bits(out[idx[rest]]), _bits(first[0][idx[rest]])) and torch.equal(_bits(lse[rest]), _bits(first[1][rest]))
    assert not torch.equal(_bits(out[idx[u]]), _bits(first[0][idx[u]]))


def test_window_u_reads_the_query_of_image_u_mod_b():
    geo = CASES['a']
    b, h, w, heads, ws = geo
    n = ws * ws
    qkv, qg, dout, bias, ref, first = _case('a', True)
    idx = R.window_index(b, h, w, ws)
    other = qg.clone()
    other[n:2 * n] = (other[n:2 * n].float() * -0.5 + 0.25).to(BF)           # image 1
    out = _launch(geo, qkv, other, bias, dout)[0]
    changed = [u for u in range(idx.shape[0]) if not torch.equal(_bits(out[idx[u]]), _bits(first[0][idx[u]]))]
    assert changed == [u for u in range(idx.shape[0]) if u % b == 1] == [1, 4, 7, 10, 13, 16]


def test_global_mode_fed_the_q_columns_is_local_mode_bit_for_bit():
    geo = CASES['c']                         # B = 1, ws = H = W
    heads = geo[3]
    c = heads * HD
    qkv, _, dout, bias = R.attn_inputs(geo, False, seed=7)
    local = _launch(geo, qkv, None, bias, dout)
    glob = _launch(geo, qkv[:, c:].contiguous(), qkv[:, :c].contiguous(), bias, dout)
    assert torch.equal(_bits(local[0]), _bits(glob[0])) and torch.equal(_bits(local[1]), _bits(glob[1]))
    # the same arithmetic in the backward too: dk | dv, and dq of the one window as d(q_global)
    assert torch.equal(_bits(local[2][:, c:]), _bits(glob[2])) and torch.equal(_bits(local[2][:, :c]), _bits(glob[3]))
    assert torch.equal(_bits(local[4]), _bits(glob[4]))


def test_refusals_name_the_entry_point_and_write_nothing():
    lib, st = _C.lib(), stream_ptr()
    b, h, w, heads, ws = 2, 8, 4, 1, 4
    c, n = heads * HD, ws * ws
    total, nw, ldb = b * h * w, 2, n
    qkv = torch.zeros(total, 3 * c, dtype=BF, device='cuda')
    bias = torch.zeros(heads * n * ldb + 4, dtype=F32, device='cuda')
    og, lg, dg, dbg = _out(total, c), _out(b * nw * heads, n, F32), _out(total, 3 * c), _out(heads * n, ldb, F32)
    ws_bytes = lib.tok_gc_attn_bwd_ws_bytes(b, h, w, heads, ws, 0, 1)
    wsb = torch.zeros(ws_bytes, dtype=torch.uint8, device='cuda')

    def fwd(c_=c, h_=h, ws_=ws, lse=lg.ptr, ldb_=ldb, bias_=bias.data_ptr(), ld=3 * c):
        return lib.tok_gc_attn_fwd(qkv.data_ptr(), ld, None, 0, bias_, ldb_, b, h_, w, c_, heads, ws_, og.ptr, c, lse, st)

    def bwd(c_=c, h_=h, ws_=ws, lse=lg.ptr, ldb_=ldb, ldd=3 * c, nbytes=ws_bytes):
        return lib.tok_gc_attn_bwd(qkv.data_ptr(), 3 * c, None, 0, bias.data_ptr(), ldb_, og.ptr, og.ptr, c, lse, b, h_, w, c_, heads,
                                   ws_, dg.ptr, ldd, None, 0, dbg.ptr, 0, wsb.data_ptr(), nbytes, st)

    def refused(rc, who, word):
        err = last_error()
        assert rc == ERR_INVALID and who in err and word in err, (rc, err)
    for call, who in ((fwd, 'tok_gc_attn_fwd'), (bwd, 'tok_gc_attn_bwd')):
        refused(call(c_=c + 8), who, 'head_dim')                 # a width that is not heads * 32
        refused(call(h_=6), who, 'multiple of the window')       # h % ws != 0
        refused(call(lse=None), who, 'null')
        refused(call(ldb_=ldb + 2), who, 'ldb')                  # not a multiple of 4
    h17 = 17 * 2
    rc = lib.tok_gc_attn_fwd(qkv.data_ptr(), 3 * c, None, 0, bias.data_ptr(), 292, 1, h17, 17, c, heads, 17, og.ptr, c, lg.ptr, st)
    refused(rc, 'tok_gc_attn_fwd', 'tokens per window')          # N = 289 > 256
    refused(fwd(bias_=bias.data_ptr() + 4), 'tok_gc_attn_fwd', 'bias')
    refused(fwd(ld=3 * c - 8), 'tok_gc_attn_fwd', 'pitches')
    refused(bwd(ldd=3 * c - 8), 'tok_gc_attn_bwd', 'ldd')
    assert bwd(nbytes=ws_bytes - 1) == -3
    assert lib.tok_gc_attn_bwd_ws_bytes(b, 6, w, heads, ws, 0, 1) == 0
    torch.cuda.synchronize()
    for t in (og, lg, dg, dbg):
        t.check('refused call')
        assert t.untouched(), 'a refused call wrote an output'


def test_dbias_partials_do_not_grow_with_the_windows():
    lib = _C.lib()
    few = lib.tok_gc_attn_bwd_ws_bytes(256, 56, 56, 2, 7, 0, 1) - lib.tok_gc_attn_bwd_ws_bytes(256, 56, 56, 2, 7, 0, 0)
    many = lib.tok_gc_attn_bwd_ws_bytes(512, 56, 56, 2, 7, 0, 1) - lib.tok_gc_attn_bwd_ws_bytes(512, 56, 56, 2, 7, 0, 0)
    assert few == many == 128 * 2 * 49 * 52 * 4                  # 128 chunk tables at most, whatever B * nW is


# ---- squeeze-excite: GELU inside, biases optional ------------------------------------------------------------------------------
def _se(x, w1, w2, b1, b2, act_kind, dout, n, hw, c, rd, want_bias_grads):
    lib, st = _C.lib(), stream_ptr()
    ld = c + 8
    xg, gg = _in(x.reshape(n * hw, c), ld), _in(dout.reshape(n * hw, c), ld)
    dev = [None if t is None else t.cuda() for t in (w1, b1, w2, b2)]
    p = [None if t is None else t.data_ptr() for t in dev]
    mean, hid, gate = _out(n, c, F32), _out(n, rd, F32), _out(n, c, F32)
    wsf = lib.tok_se_act_ws_floats(n, hw, c, rd)
    ws = GuardedSpan(wsf, F32, GUARD, nan_guard=True)
    _C.check(lib.tok_se_act_fwd(xg.ptr, n, hw, c, ld, rd, 0, act_kind, p[0], p[1], p[2], p[3], mean.ptr, hid.ptr, gate.ptr, ws.ptr,
                                st), 'se fwd')
    dw1, dw2 = _out(rd, c, F32), _out(c, rd, F32)
    db1, db2 = (_out(1, rd, F32), _out(1, c, F32)) if want_bias_grads else (None, None)
    dx = _out(n * hw, ld)
    ws2 = GuardedSpan(wsf, F32, GUARD, nan_guard=True)
    _C.check(lib.tok_se_act_bwd(gg.ptr, xg.ptr, n, hw, c, ld, rd, 0, act_kind, p[0], p[2], mean.ptr, hid.ptr, gate.ptr, dw1.ptr,
                                None if db1 is None else db1.ptr, dw2.ptr, None if db2 is None else db2.ptr, 0, dx.ptr, 0, ws2.ptr,
                                st), 'se bwd')
    torch.cuda.synchronize()
    for buf in (xg, gg, mean, hid, gate, ws, dw1, dw2, db1, db2, dx, ws2):
        if buf is not None:
            buf.check('se')
    dxv, pads_ok = _value(dx, n * hw, ld, c)
    assert pads_ok
    val = lambda t: None if t is None else t.value()           # noqa: E731
    return gate.value().view(n, c), dxv.view(n, hw, c), dw1.value().view(rd, c), dw2.value().view(c, rd), val(db1), val(db2)


@pytest.mark.parametrize('biased', [False, True], ids=['nobias', 'bias'])
@pytest.mark.parametrize('act', ['gelu', 'relu'])
@pytest.mark.parametrize('c,rd', [(16, 8), (64, 16)])
def test_se_with_gelu_and_without_biases(c, rd, act, biased):
    n, hw = 2, 9
    g = torch.Generator().manual_seed(c + rd)
    x = torch.randn(n, hw, c, generator=g).to(BF)
    dout = torch.randn(n, hw, c, generator=g).to(BF)
    w1, w2 = torch.randn(rd, c, generator=g) * c ** -0.5 * 2, torch.randn(c, rd, generator=g) * rd ** -0.5 * 2
    b1, b2 = (torch.randn(rd, generator=g) * 0.3, torch.randn(c, generator=g) * 0.3) if biased else (None, None)
    gate, dx, dw1, dw2, db1, db2 = _se(x, w1, w2, b1, b2, 1 if act == 'gelu' else 0, dout, n, hw, c, rd, biased)
    out_r, gate_r, dx_r, (dw1_r, dw2_r, db1_r, db2_r) = R.se_ref(x, w1, w2, b1, b2, act, dout)
    tag = 'se_act_contract/c%d_%s_%s' % (c, act, 'bias' if biased else 'nobias')
    # the gate: fp32 chains of length hw, c and rd and two transcendentals (GELU's polynomial is 3e-7 in Phi): 1e-5 of a value in (0, 1)
    assert_bounded(gate, gate_r, torch.ones_like(gate_r), 0.0, 1e-5, 'gate', tag)
    # dx: one bf16 rounding of dout * s + dmean / hw, fp32 chains behind it
    mag = dout.double().abs() * gate_r[:, None, :] + (dx_r - dout.double() * gate_r[:, None, :]).abs()
    assert_bounded(dx, dx_r, mag + 1e-3 * mag.max(), 2.0 ** -8, 1e-4, 'dx', tag)
    for mine, want, what in ((dw1, dw1_r, 'dw1'), (dw2, dw2_r, 'dw2'), (db1, db1_r, 'db1'), (db2, db2_r, 'db2')):
        if want is None:
            assert mine is None
            continue
        # fp32 sums over images, pixels and channels of products of O(1) terms: 1e-4 of the largest element
        assert_bounded(mine.view(want.shape), want, torch.full_like(want, float(want.abs().max())), 1e-4, 1e-4, what, tag)


def test_se_act_relu_with_biases_is_the_old_entry_point_bit_for_bit():
    lib, st = _C.lib(), stream_ptr()
    n, hw, c, rd = 2, 9, 16, 8
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n * hw, c, generator=g).to(BF).cuda()
    w1, b1 = torch.randn(rd, c, generator=g).cuda(), torch.randn(rd, generator=g).cuda()
    w2, b2 = torch.randn(c, rd, generator=g).cuda(), torch.randn(c, generator=g).cuda()
    res = []
    for new in (False, True):
        mean, hid, gate = (torch.empty(n, k, dtype=F32, device='cuda') for k in (c, rd, c))
        ws = torch.empty(lib.tok_se_act_ws_floats(n, hw, c, rd), dtype=F32, device='cuda')
        args = (w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), mean.data_ptr(), hid.data_ptr(), gate.data_ptr(),
                ws.data_ptr(), st)
        if new:
            _C.check(lib.tok_se_act_fwd(x.data_ptr(), n, hw, c, c, rd, 0, 0, *args), 'new')
        else:
            _C.check(lib.tok_se_fwd(x.data_ptr(), n, hw, c, c, rd, *args), 'old')
        torch.cuda.synchronize()
        res.append((mean.cpu(), hid.cpu(), gate.cpu()))
    for a, bb in zip(*res):
        assert torch.equal(_bits(a), _bits(bb))


def test_se_act_refusals():
    lib, st = _C.lib(), stream_ptr()
    t = torch.zeros(64, dtype=F32, device='cuda')
    p = t.data_ptr()
    assert lib.tok_se_act_fwd(p, 1, 1, 8, 8, 4, 0, 2, p, None, p, None, p, p, p, p, st) == ERR_INVALID
    assert 'tok_se_act_fwd' in last_error() and 'activation' in last_error()
    assert lib.tok_se_act_fwd(p, 1, 1, 8, 8, 4, 0, 1, p, p, p, None, p, p, p, p, st) == ERR_INVALID
    assert 'tok_se_act_fwd' in last_error() and 'both' in last_error()
    assert lib.tok_se_act_bwd(p, p, 1, 1, 12, 16, 4, 0, 1, p, p, p, p, p, p, None, p, None, 0, p, 0, p, st) == ERR_INVALID
    assert 'tok_se_act_bwd' in last_error()
