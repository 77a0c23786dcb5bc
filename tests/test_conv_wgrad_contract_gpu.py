"""The convolution weight gradient (csrc/conv_wgrad.hip, the stem form of csrc/stem.hip) across the contract of include/tok.h,
element by element against fp64 - the companion of tests/test_conv_contract_gpu.py, whose guards, references and conventions it
shares.

make_plan is restated below (every threshold at its default); each case names the kernel it is meant for, the test asserts the
restated plan gives that name and that tok_conv_wgrad_ws_bytes / tok_conv_wgrad_bias_ws_bytes / tok_conv_wgrad_bias_ok equal the
restated values.  The workspace is exactly as many bytes as the query returns, its guard starts at that byte; dw is exactly
k_real x r x s x c_real floats, so a store of a padded row or channel lands in its guard.

Bound: dw and dbias are fp32 sums of exact products, a = 0, b = 2 d 2^-24 of the magnitude term, d the dependent chain: the rows
of one split chunk (any order inside the MFMA), the split slabs folded after them, one more under +=.

Host cost, measured on 16 CPU threads: the fp64 references of all cases take under 2 s (pointwise layers are a matmul), the
slowest case (the 200 704-row layer of the 256 x 256 kernel) 1 s with its comparisons."""
import ctypes
from collections import namedtuple

import pytest
import torch

from helpers import BF, ERR_INVALID, ERR_WORKSPACE, F32, U8, U32, assert_bounded, cdiv, conv_desc as mk, gin, gout, halo_guard, last_error
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu

# ---- make_plan (csrc/conv_wgrad.hip) and stem_wgrad_serves (csrc/stem.hip), restated -------------------------------------------
Plan = namedtuple('Plan', 'kernel TN TK tilesN tilesK splitM mchunk MS ring')
TAPS_WGS, TWO_BUF_WGS = 256, 1024


def _split(m, target, tiles, ms, cap):
    split = min(cdiv(target, tiles), cdiv(m, 8 * ms), cap)
    split = max(split, 1)
    chunk = cdiv(cdiv(m, split), ms) * ms
    return cdiv(m, chunk), chunk


def stem_wgrad_serves(d):
    if not (d.c == 4 and d.r == 7 and d.s == 7 and d.s_pad == 8 and d.stride == 2 and d.pad == 3):
        return False
    return d.k % 8 == 0 and d.k <= 64 and d.w % 2 == 0 and d.n * cdiv(d.p, 8) * cdiv(d.q, 16) >= 16


def make_plan(d):
    ktot, m = d.r * d.s_pad * d.c, d.n * d.p * d.q
    small = d.n * d.h * d.w * d.c * 2 < 0x40000000 and m * d.k * 2 < 0x40000000
    same3 = d.r == 3 and d.s == 3 and d.s_pad == 3 and d.stride == 1 and d.pad == 1 and small
    w64 = d.c % 64 == 0 and d.k % 64 == 0
    w48 = not w64 and d.c % 48 == 0 and d.k % 48 == 0 and same3
    if d.c != 4 and (w64 or w48) and d.r == 3 and d.s == 3:
        tn = 64 if w64 else 48
        tiles_n, tiles_k = cdiv(d.k, tn), cdiv(d.c, tn)
        split, chunk = _split(m, TAPS_WGS, tiles_n * tiles_k, 32, 512)
        same = d.stride == 1 and d.pad == 1 and d.p == d.h and d.q == d.w and small
        return Plan(f'winp<{tn}>' if same else 'taps', tn, tn, tiles_n, tiles_k, split, chunk, 32, False)
    if d.c != 4 and d.r == 1 and d.s == 1 and d.stride == 1 and d.pad == 0:
        if d.k <= 64:
            tn, tk = 64, (256 if ktot >= 256 else 128 if ktot >= 128 else 64)
        elif ktot <= 64:
            tn, tk = (256 if d.k >= 256 else 128), 64
        else:
            tn, tk = 128, 128
        if d.k >= 256 and ktot >= 256 and m >= 200000 and cdiv(d.k, 256) * cdiv(ktot, 256) * 65536 * 2 <= d.k * ktot * 3:
            tn, tk = 256, 256
        tiles_n, tiles_k = cdiv(d.k, tn), cdiv(ktot, tk)
        per_cu = (160 * 1024) // (3 * 32 * (tn + tk) * 2)
        split, chunk = _split(m, 256 * min(per_cu, 2), tiles_n * tiles_k, 32, 512)
        return Plan(f'ring8<{tn},{tk}>' if tn == tk == 256 else f'ring<{tn},{tk}>', tn, tk, tiles_n, tiles_k, split, chunk, 32, True)
    tn, tk = (128 if d.k >= 128 else 64), (128 if ktot >= 128 else 64)
    tiles_n, tiles_k = cdiv(d.k, tn), cdiv(ktot, tk)
    ms = 64 if (m >= 100000 and tn == 128 and tk == 128) else 32
    split, chunk = _split(m, TWO_BUF_WGS, tiles_n * tiles_k, ms, 512 if (d.c == 4 and tiles_n * tiles_k <= 2) else 256)
    if stem_wgrad_serves(d):
        return Plan('stem_wgrad', tn, tk, tiles_n, tiles_k, split, chunk, ms, False)
    return Plan(f'2buf<{tn},{tk},{"c4," if d.c == 4 else ""}ms{ms}>', tn, tk, tiles_n, tiles_k, split, chunk, ms, False)


def dw_chain(d, p):
    """rows of one split chunk (the stem kernel: the 8 x 16 pixel tiles one of its `splitM` workgroups walks), then the slabs"""
    rows = p.mchunk
    if p.kernel == 'stem_wgrad':
        rows = max(rows, cdiv(d.n * cdiv(d.p, 8) * cdiv(d.q, 16), p.splitM) * 128)
    return rows + p.splitM


# (id, (n, h, w, c, k, r, stride, pad), k_real, c_real, kernel)
WGRAD_CASES = [
    ('winp64', (2, 16, 16, 64, 64, 3, 1, 1), 64, 64, 'winp<64>'),
    ('winp64_two_tiles', (2, 56, 56, 64, 128, 3, 1, 1), 128, 64, 'winp<64>'),
    ('winp64_7x7_deep', (1, 7, 7, 512, 512, 3, 1, 1), 512, 512, 'winp<64>'),                 # n = 1, 49 rows: one ragged chunk
    ('winp64_real', (5, 14, 14, 64, 64, 3, 1, 1), 60, 58, 'winp<64>'),                      # k_real < k, c_real < c
    ('winp48', (2, 30, 26, 96, 48, 3, 1, 1), 48, 96, 'winp<48>'),
    ('winp48_ragged', (3, 9, 33, 48, 48, 3, 1, 1), 48, 48, 'winp<48>'),
    ('taps_s2', (2, 17, 19, 64, 128, 3, 2, 1), 128, 64, 'taps'),                             # per-tap form: stride 2, odd extents
    ('taps_1x1_out', (70, 2, 2, 64, 128, 3, 2, 1), 128, 64, 'taps'),
    ('ring64x64', (2, 16, 16, 64, 64, 1, 1, 0), 64, 64, 'ring<64,64>'),
    ('ring64x64_tiny', (1, 5, 3, 64, 64, 1, 1, 0), 64, 64, 'ring<64,64>'),                   # 15 rows
    ('ring64x128', (2, 16, 16, 128, 64, 1, 1, 0), 64, 128, 'ring<64,128>'),
    ('ring64x256', (2, 16, 16, 256, 64, 1, 1, 0), 50, 256, 'ring<64,256>'),
    ('ring128x64', (2, 16, 16, 64, 128, 1, 1, 0), 121, 60, 'ring<128,64>'),
    ('ring256x64', (3, 9, 11, 64, 256, 1, 1, 0), 256, 64, 'ring<256,64>'),
    ('ring128x128', (2, 14, 14, 384, 1536, 1, 1, 0), 1530, 384, 'ring<128,128>'),
    ('ring128x128_tokens', (3, 1, 1, 2048, 1000, 1, 1, 0), 1000, 2048, 'ring<128,128>'),     # 3 rows, deepest reduction
    ('ring8_256x256', (64, 56, 56, 256, 256, 1, 1, 0), 256, 256, 'ring8<256,256>'),          # 200 704 rows: the default threshold
    ('2buf64x64', (2, 8, 8, 8, 24, 3, 1, 1), 24, 8, '2buf<64,64,ms32>'),
    ('2buf128x128', (5, 13, 15, 40, 136, 3, 1, 1), 130, 36, '2buf<128,128,ms32>'),
    ('2buf128x64_1x1_s2', (3, 14, 14, 64, 256, 1, 2, 0), 256, 64, '2buf<128,64,ms32>'),
    ('2buf64x128_patch', (2, 16, 16, 96, 40, 2, 2, 0), 40, 96, '2buf<64,128,ms32>'),
    ('2buf128x128_ms64', (8, 128, 128, 40, 136, 3, 1, 1), 136, 40, '2buf<128,128,ms64>'),    # >= 100 000 rows: 64 rows per barrier
    ('2buf_c4', (2, 33, 35, 4, 64, 7, 2, 3), 64, 3, '2buf<64,128,c4,ms32>'),                 # odd width: off the stem window kernel
    ('stem_wgrad', (4, 70, 72, 4, 64, 7, 2, 3), 64, 3, 'stem_wgrad'),
    ('stem_wgrad_k32', (3, 64, 96, 4, 32, 7, 2, 3), 30, 3, 'stem_wgrad'),
]
ROUTES_WGRAD = {'winp<64>', 'winp<48>', 'taps', 'ring<64,64>', 'ring<64,128>', 'ring<64,256>', 'ring<128,64>', 'ring<256,64>',
                'ring<128,128>', 'ring8<256,256>', '2buf<64,64,ms32>', '2buf<128,128,ms32>', '2buf<128,64,ms32>',
                '2buf<64,128,ms32>', '2buf<128,128,ms64>', '2buf<64,128,c4,ms32>', 'stem_wgrad'}


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
