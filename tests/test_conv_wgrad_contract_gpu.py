"""The convolution weight gradient (csrc/conv_wgrad.hip, the stem form of csrc/stem.hip) across the contract of include/tok.h,
element by element against fp64 - the companion of tests/test_conv_contract_gpu.py, whose guards, references and conventions it
shares.

make_plan is restated in tests/conv_wgrad_plan_ref.py (every threshold at its default), which also lists the cases; each case
names the kernel it is meant for, the test asserts the restated plan gives that name and that tok_conv_wgrad_ws_bytes /
tok_conv_wgrad_bias_ws_bytes / tok_conv_wgrad_bias_ok equal the restated values.  The workspace is exactly as many bytes as the query returns, its guard starts at that byte; dw is exactly
k_real x r x s x c_real floats, so a store of a padded row or channel lands in its guard.

Bound: dw and dbias are fp32 sums of exact products, a = 0, b = 2 d 2^-24 of the magnitude term, d the dependent chain: the rows
of one split chunk (any order inside the MFMA), the split slabs folded after them, one more under +=.

Host cost, measured on 16 CPU threads: the fp64 references of all cases take under 2 s (pointwise layers are a matmul), the
slowest case (the 200 704-row layer of the 256 x 256 kernel) 1 s with its comparisons."""
import ctypes

import pytest
import torch

from conv_wgrad_plan_ref import ROUTES_WGRAD, WGRAD_CASES, make_plan
from helpers import BF, ERR_INVALID, ERR_WORKSPACE, F32, U8, U32, assert_bounded, cdiv, conv_desc as mk, gin, gout, halo_guard, last_error
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu

def dw_chain(d, p):
    """rows of one split chunk (the stem kernel: the 8 x 16 pixel tiles one of its `splitM` workgroups walks), then the slabs"""
    rows = p.mchunk
    if p.kernel == 'stem_wgrad':
        rows = max(rows, cdiv(d.n * cdiv(d.p, 8) * cdiv(d.q, 16), p.splitM) * 128)
    return rows + p.splitM


def test_every_wgrad_route_has_a_case():
    assert {c[4] for c in WGRAD_CASES} == ROUTES_WGRAD


@pytest.mark.parametrize('case', WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_conv_wgrad_contract(case):
    name, geo, k_real, c_real, kernel = case
    lib, st = _C.lib(), stream_ptr()
    n, h, w, c, k, r, stride, pad = geo
    d, tag = mk(*geo), f'conv_contract/wgrad/{name}'
    D = ctypes.byref(d)
    p = make_plan(d)
    assert p.kernel == kernel
    slab = k * r * d.s_pad * c
    ws_bytes = p.splitM * slab * 4
    assert lib.tok_conv_wgrad_ws_bytes(D) == ws_bytes
    assert lib.tok_conv_wgrad_bias_ok(D) == int(p.ring)
    assert lib.tok_conv_wgrad_bias_ws_bytes(D) == ws_bytes + p.splitM * k * 4

    g = torch.Generator().manual_seed(3 * sum(geo) + len(name))
    x = torch.randn(n, h, w, c, generator=g).to(BF)
    if c == 4:
        x[..., 3] = 0
    dy = torch.randn(n, d.p, d.q, k, generator=g).to(BF)
    s_real = d.s
    numel = k_real * r * s_real * c_real
    old = torch.randn(numel, generator=g)
    old_b = torch.randn(k_real, generator=g)
    xg, gg = gin(x, halo_guard(pad, w, c, c)), gin(dy, 128 * k)
    outs = []

    def run(acc, init=None, bias_acc=None, short=0):
        dw = gout(numel, F32, 128 * r * s_real * c_real, init=init)
        outs.append((dw, 'dw'))
        if bias_acc is None:
            ws = gout(ws_bytes - short, U8, 1 << 16)
            outs.append((ws, 'ws'))
            return dw, None, lib.tok_conv_wgrad(D, xg.ptr, gg.ptr, dw.ptr, k_real, c_real, ws.ptr, ws_bytes - short, acc, st)
        nb = ws_bytes + p.splitM * k * 4
        ws, db = gout(nb - short, U8, 1 << 16), gout(k_real, F32, 128, init=old_b if bias_acc else None)
        outs.extend([(ws, 'ws'), (db, 'dbias')])
        return dw, db, lib.tok_conv_wgrad_bias(D, xg.ptr, gg.ptr, dw.ptr, k_real, c_real, ws.ptr, nb - short, acc, db.ptr,
                                               bias_acc, st)

    a0, _, rc = run(0)
    _C.check(rc, 'wgrad')
    a1, _, rc = run(0)
    _C.check(rc, 'wgrad(again)')
    a2, _, rc = run(1, init=old)
    _C.check(rc, 'wgrad(+=)')
    torch.cuda.synchronize()

    xd, gd = x.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2)
    kw = dict(stride=stride, padding=pad)
    cut = lambda t: t.permute(0, 2, 3, 1)[:k_real, :, :, :c_real].reshape(-1)          # noqa: E731  [k][c][r][s] -> [k_real][r][s][c_real]
    if r == 1 and stride == 1 and pad == 0:                # a matmul
        x2, g2 = x.double().view(-1, c), dy.double().view(-1, k)
        ref, mag = (g2.t() @ x2)[:k_real, :c_real].reshape(-1), (g2.abs().t() @ x2.abs())[:k_real, :c_real].reshape(-1)
    else:
        ref = cut(torch.nn.grad.conv2d_weight(xd, (k, c, r, s_real), gd, **kw))
        mag = cut(torch.nn.grad.conv2d_weight(xd.abs(), (k, c, r, s_real), gd.abs(), **kw))
    chain = dw_chain(d, p)
    assert_bounded(a0.value(), ref, mag, 0.0, 2 * chain * U32, 'dw', tag)
    assert torch.equal(a1.value(), a0.value()), 'not bit-reproducible'
    o64 = old.double()
    assert_bounded(a2.value(), o64 + ref, o64.abs() + mag, 0.0, 2 * (chain + 1) * U32, 'dw +=', tag)

    # one byte short: refused, nothing written
    z, _, rc = run(0, short=1)
    assert rc == ERR_WORKSPACE and 'tok_conv_wgrad' in last_error(), (rc, last_error())
    torch.cuda.synchronize()
    assert z.untouched() and outs[-1][0].untouched()

    if p.ring:
        # the bias gradient (column sums of dy) from the same launch, = and +=; dw bit-identical to tok_conv_wgrad
        gk = dy.double().reshape(-1, k)[:, :k_real]
        for acc, bias_acc in ((0, 0), (1, 1), (0, 1)):
            dw, db, rc = run(acc, init=old if acc else None, bias_acc=bias_acc)
            _C.check(rc, 'wgrad_bias')
            torch.cuda.synchronize()
            assert torch.equal(dw.value(), (a2 if acc else a0).value()), 'dw of tok_conv_wgrad_bias differs from tok_conv_wgrad'
            ob = old_b.double() * bias_acc
            assert_bounded(db.value(), ob + gk.sum(0), ob.abs() + gk.abs().sum(0), 0.0, 2 * (chain + bias_acc) * U32,
                           f'dbias (acc {bias_acc})', tag)
        z, db, rc = run(0, bias_acc=0, short=1)
        assert rc == ERR_WORKSPACE, (rc, last_error())
        torch.cuda.synchronize()
        assert z.untouched() and db.untouched()
    else:
        z, db, rc = run(0, bias_acc=0)
        assert rc == ERR_INVALID and 'tok_conv_wgrad_bias' in last_error(), (rc, last_error())
        torch.cuda.synchronize()
        assert z.untouched() and db.untouched()

    for buf, what in outs + [(xg, 'x'), (gg, 'dy')]:
        buf.check(f'{name}: {what}')


def test_conv_wgrad_refusals():
    lib, st = _C.lib(), stream_ptr()
    d = mk(2, 16, 16, 64, 64, 3, 1, 1)
    D = ctypes.byref(d)
    src = gin(torch.zeros(2 * 16 * 16 * 64, dtype=BF), 1024)
    dw, ws = gout(64 * 9 * 64, F32, 1024), gout(lib.tok_conv_wgrad_ws_bytes(D), U8, 1024)
    n_ws = ws.numel

    def refused(rc, code=ERR_INVALID):
        assert rc == code and 'tok_conv_wgrad' in last_error(), (rc, last_error())
        torch.cuda.synchronize()
        assert dw.untouched() and ws.untouched()
    refused(lib.tok_conv_wgrad(D, src.ptr, src.ptr, dw.ptr, 72, 64, ws.ptr, n_ws, 0, st))       # k_real > k
    refused(lib.tok_conv_wgrad(D, src.ptr, src.ptr, dw.ptr, 64, 65, ws.ptr, n_ws, 0, st))       # c_real > c
    refused(lib.tok_conv_wgrad(D, None, src.ptr, dw.ptr, 64, 64, ws.ptr, n_ws, 0, st))
    refused(lib.tok_conv_wgrad(D, src.ptr, src.ptr, dw.ptr, 64, 64, None, n_ws, 0, st))
    bad = _C.ConvDesc(2, 16, 16, 60, 64, 3, 3, 16, 16, 1, 1, 3)
    refused(lib.tok_conv_wgrad(ctypes.byref(bad), src.ptr, src.ptr, dw.ptr, 64, 60, ws.ptr, n_ws, 0, st))
    bad = _C.ConvDesc(2, 16, 16, 64, 64, 3, 3, 16, 16, 1, 1, 8)
    refused(lib.tok_conv_wgrad(ctypes.byref(bad), src.ptr, src.ptr, dw.ptr, 64, 64, ws.ptr, n_ws, 0, st))
    refused(lib.tok_conv_wgrad(D, src.ptr, src.ptr, dw.ptr, 64, 64, ws.ptr, n_ws - 1, 0, st), ERR_WORKSPACE)
    for b in (dw, ws, src):
        b.check('refusals')
