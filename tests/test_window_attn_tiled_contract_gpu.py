"""The tiled window-attention family (csrc/window_attn_tiled.hip: windows of 18 x 18 tokens and up, on 64-token MFMA tiles)
across the contract of include/tok.h, element by element against the fp64 reference of tests/window_attn_ref.py with the bounds
of its MFMA path: q and k are bf16 MFMA operands here as for windows of up to 64 tokens, so Delta_i = scale_h 2^-8 max_j sum_d
|qn||kn| applies (uses_mfma is patched for these windows; no bound is changed).  Buffers are guarded as in
tests/test_window_attn_contract_gpu.py.  The device backward gets the device forward's log-sum-exp, as in training.

The case with head 0 at the clamped scale of 100 (b 2, 18 x 36, N = 324) is why the family forms its cosines from bf16 PAIRS:
emulate_device of tests/window_attn_ref.py, an exact kernel with single-bf16 qn and kn, misses the 3e-2 row gates there (dk 3.9e-2
... 8.9e-2 over the seeds 1 ... 12, 7.6e-2 at this one; dv 9.9e-2) and is at 2e-3 ... 4e-3 with exact cosines."""
import pytest
import torch

from helpers import BF, ERR_INVALID, ERR_WORKSPACE, F32, SENTINEL, Guarded, _INT_OF, cdiv, last_error
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr
import window_attn_ref
from window_attn_ref import HD, WinRef, check_result, make_inputs

pytestmark = pytest.mark.gpu
P = lambda t: None if t is None else t.data_ptr()       # noqa: E731
R = 2                                                   # SCRATCH_ROWS of csrc/window_attn_tiled.hip


def _all_written(g, what):
    left = int((g.buf.view(_INT_OF[g.dtype])[:g.rows, :g.cols] == SENTINEL[g.dtype]).sum())
    assert left == 0, f'{what}: {left} owned elements never written'
    assert torch.isfinite(g.view.float()).all(), f'{what}: not finite'


def _launch(dims, qkv, dout, ls, bias, mask):
    """forward + backward on guarded buffers: qkv at pitch 3c + 8 (forward) / 3c + 16 (backward, the pitch of dqkv) with NaN
    pads, NaN guard rows behind qkv and dout, sentinels in every output, its pads and its guard row, a guarded workspace"""
    b, h, w, heads, ws, shift = dims
    lib, st = _C.lib(), stream_ptr()
    c, n, nw, rows = heads * HD, ws * ws, (h // ws) * (w // ws), b * h * w
    ldq, ldd = 3 * c + 8, 3 * c + 16
    dev = [t if t is None else t.cuda() for t in (ls, bias, mask)]
    qg = Guarded(rows, 3 * c, ldq, init=qkv.cuda(), nan_pad=True)
    og = Guarded(rows, c)
    lg = Guarded(b * nw * heads, n, dtype=F32)
    _C.check(lib.tok_window_attn_fwd(qg.ptr, b, h, w, c, heads, ws, shift, ldq, P(dev[0]), P(dev[1]), P(dev[2]), og.ptr, lg.ptr,
                                     st), 'fwd')
    torch.cuda.synchronize()
    r = lib.tok_window_attn_bwd_rows(b, h, w, heads, ws)
    assert r == min(b, R) * nw
    wsb = int(lib.tok_window_attn_tiled_ws_bytes(b, h, w, heads, ws))
    assert wsb > 0 and wsb % 4 == 0
    q2 = Guarded(rows, 3 * c, ldd, init=qkv.cuda(), nan_pad=True)
    gg = Guarded(rows, c, init=dout.cuda(), nan_pad=True)
    dg = Guarded(rows, 3 * c, ldd)
    sg, pg, wg = Guarded(r, heads * n * n, dtype=F32), Guarded(r, heads, dtype=F32), Guarded(1, wsb // 4, dtype=F32)
    _C.check(lib.tok_window_attn_tiled_bwd(q2.ptr, gg.ptr, b, h, w, c, heads, ws, shift, ldd, P(dev[0]), P(dev[1]), P(dev[2]), lg.ptr,
                                           dg.ptr, sg.ptr, pg.ptr, wg.ptr, wsb, st), 'bwd')
    torch.cuda.synchronize()
    for g, what in ((qg, 'qkv'), (og, 'out'), (lg, 'lse'), (q2, 'qkv'), (gg, 'dout'), (dg, 'dqkv'), (sg, 'ds_scratch'),
                    (pg, 'dscale_part'), (wg, 'workspace')):
        g.check(what)
        if g not in (qg, q2, gg, wg):
            _all_written(g, what)
    return og.value(), lg.value(), dg.value(), sg, pg


def _case(tag, dims, seed, colsum=False, **kw):
    b, heads, n = dims[0], dims[3], dims[4] ** 2
    qkv, dout, ls, bias, mask = make_inputs(*dims, seed=seed, **kw)
    out, lse, dqkv, sg, pg = _launch(dims, qkv, dout, ls, bias, mask)
    ref = WinRef(qkv, dout, *dims, ls, bias, mask, bpw=cdiv(b, min(b, R)))
    scr, part = sg.value(), pg.value()                                    # every scratch row is checked on its own ...
    dbias = scr.double().sum(0).view(heads, n, n)                         # ... and the fp64 host fold of the rows
    dls = part.double().sum(0)
    check_result(f'winattn_tiled/{tag}', ref, out, lse, dqkv, dbias, dls, scr, part)
    if colsum:                                                            # ... and the fold the engine does
        lib, st = _C.lib(), stream_ptr()
        red, redl = Guarded(1, heads * n * n, dtype=F32), Guarded(1, heads, dtype=F32)
        _C.check(lib.tok_colsum_f32(sg.ptr, sg.rows, heads * n * n, red.ptr, 0, st), 'colsum')
        _C.check(lib.tok_colsum_f32(pg.ptr, pg.rows, heads, redl.ptr, 0, st), 'colsum')
        torch.cuda.synchronize()
        red.check('d(bias) fold')
        redl.check('d(logit_scale) fold')
        check_result(f'winattn_tiled/{tag}_colsum', ref, out, lse, dqkv, red.value().double().view(heads, n, n),
                     redl.value().double().view(heads))


CASES = [   # b, h, w, heads, ws, shift, seed, inputs
    (1, 18, 18, 1, 18, 0, 1, {}),                      # N = 324: five full tiles and a tail of 4 keys / queries, one window
    (2, 18, 36, 2, 18, 9, 6, {'ls0': 5.0}),           # the tail with roll and mask, two windows, head 0 clamped (scale 100)
    (1, 24, 24, 1, 24, 0, 3, {}),                      # N = 576: nine exact tiles
    (1, 48, 24, 2, 24, 12, 4, {'sharp_head': 1}),      # shifted; rows nearly one-hot, whole key tiles behind the mask
    (R + 1, 18, 18, 1, 18, 0, 5, {}),                  # image groups of two and one
]


@pytest.mark.parametrize('b,h,w,heads,ws,shift,seed,kw', CASES, ids=[f'b{c[0]}_{c[1]}x{c[2]}_ws{c[4]}_s{c[5]}' for c in CASES])
def test_contract(monkeypatch, b, h, w, heads, ws, shift, seed, kw):
    monkeypatch.setattr(window_attn_ref, 'uses_mfma', lambda ws: True)
    _case(f'b{b}_{h}x{w}_ws{ws}_h{heads}_s{shift}', (b, h, w, heads, ws, shift), seed, colsum=(shift == 9), **kw)


def test_reruns_are_bit_identical_and_refusals_write_nothing():
    dims = (2, 18, 36, 2, 18, 9)
    inputs = make_inputs(*dims, seed=2, ls0=5.0)
    first, again = _launch(dims, *inputs), _launch(dims, *inputs)
    for a, bb in zip(first, again):
        a, bb = (t.value() if isinstance(t, Guarded) else t for t in (a, bb))
        assert torch.equal(a.view(_INT_OF[a.dtype]), bb.view(_INT_OF[bb.dtype]))
    lib, st = _C.lib(), stream_ptr()
    b, h, w, heads, ws, shift = dims
    c, n, nw, rows = heads * HD, ws * ws, 2, b * h * w
    qkv = torch.zeros(rows + 1, 3 * c, dtype=BF, device='cuda')
    ls, bias, mask = torch.zeros(heads, device='cuda'), torch.zeros(heads, n, n, device='cuda'), torch.zeros(nw, n, n, device='cuda')
    wsb = int(lib.tok_window_attn_tiled_ws_bytes(b, h, w, heads, ws))
    outs = [Guarded(rows, c), Guarded(b * nw * heads, n, dtype=F32), Guarded(rows, 3 * c), Guarded(R * nw, heads * n * n, dtype=F32),
            Guarded(R * nw, heads, dtype=F32), Guarded(1, wsb // 4, dtype=F32)]
    og, lg, dg, sg, pg, wg = outs

    def fwd(q=qkv.data_ptr(), ls=ls, bias=bias, out=og.ptr):
        return lib.tok_window_attn_fwd(q, b, h, w, c, heads, ws, shift, 3 * c, P(ls), P(bias), P(mask), out, lg.ptr, st)

    def bwd(q=qkv.data_ptr(), dout=qkv.data_ptr(), ls=ls, bias=bias, wsb=wsb):
        return lib.tok_window_attn_tiled_bwd(q, dout, b, h, w, c, heads, ws, shift, 3 * c, P(ls), P(bias), P(mask), lg.ptr, dg.ptr,
                                             sg.ptr, pg.ptr, wg.ptr, wsb, st)
    for call, kw, status, names in ((bwd, {'wsb': wsb - 1}, ERR_WORKSPACE, 'ws_bytes'),
                                    (bwd, {'q': qkv.data_ptr() + 8}, ERR_INVALID, 'qkv'),
                                    (fwd, {'q': qkv.data_ptr() + 8}, ERR_INVALID, 'qkv'),
                                    (bwd, {'ls': None, 'bias': None}, ERR_INVALID, 'plain mode'),
                                    (fwd, {'ls': None, 'bias': None}, ERR_INVALID, 'plain mode'),
                                    (bwd, {'dout': None}, ERR_INVALID, 'dout'),
                                    (fwd, {'out': None}, ERR_INVALID, 'out')):
        rc, err = call(**kw), last_error()
        assert rc == status, (rc, status, err)
        assert names in err, (names, err)
    torch.cuda.synchronize()
    for g in outs:
        assert bool((g.buf.view(_INT_OF[g.dtype]) == SENTINEL[g.dtype]).all()), 'a refused call wrote to an output'
