"""The convolution kernels (csrc/conv_igemm.hip, pw_gemm.hip, gemm256.hip, conv_win.hip, conv_s2d.hip, stem.hip and the epilogues
of unit3) across the contract of include/tok.h: forward and data gradient, element by element against fp64 (the weight gradient
is tests/test_conv_wgrad_contract_gpu.py).

Guards.  Every operand sits in a helpers.GuardedSpan: a guard of at least one full halo and at least one 128-row tile in front
AND behind (halos reach backwards).  Inputs carry NaN there, so a value the kernel does not own that reaches a result - even
multiplied by a zero weight - fails the bound; outputs carry sentinel bits, asserted unchanged after every call.

Routes.  The library's route is restated in tests/conv_route_ref.py (at the thresholds tests/conftest.py sets:
TOK_CONV_WIN_MIN_TILES = TOK_CONV_S2D_MIN_TILES = 1, everything else default; tests/test_conv_route.py compares it with the
library's queries without a GPU).  Every case names the kernel it is meant for; the test asserts that the restatement gives that
name and that the library's row queries equal the restated ones, so a routing change breaks a test instead of silently moving
its coverage.  ROUTES_FWD / ROUTES_DGRAD list what must be covered.

Bounds (derived, not fitted).  bf16 results of an fp32 accumulator: |err| <= 2^-8 |ref| + d 2^-24 mag, `mag` the same operation on
absolute values, d the fp32 additions on the longest path into one output: the whole reduction length (MFMA's internal order is
unspecified) plus one per epilogue term (bias, the old value under +=, shortcut, dsub, BatchNorm's fma).  fp32 sums of n stored
values in any order: 2 n 2^-24 of the sum of magnitudes, n the values one partial row holds (restated from the grid).

Statistics.  Every kernel here sums the STORED bf16 values (conv_igemm.hip, pw_gemm.hip, gemm256.hip, conv_win_epilogue.inc and
stem.hip all reduce bf2f(o[e]) of the vector they store), which is what include/tok.h states; so the fold of the rows is compared
with fp64 sums of the kernel's own output within the summation bound alone.

Host cost, measured on 16 CPU threads: the fp64 references of all forward cases take 6 s, of all data-gradient cases 2.5 s
(pointwise layers are a matmul); with the element-wise comparisons both contract modules together run in 17 s, the slowest
case (the 103 488-row ring data gradient with its seven epilogues) in 3 s."""
import ctypes
import pytest
import torch
import torch.nn.functional as F

from conv_route_ref import ACT_ROUTES, ROUTES_DGRAD, ROUTES_FWD, pick_bn, pw_serves, route_dgrad, route_fwd
from helpers import (A_BF, BF, ERR_INVALID, F32, U8, U32, assert_bounded, cdiv, conv_desc as mk, gin, gout, halo_guard, last_error,
                     pack_bits, unpack_bits)
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
GELU_PHI = 3e-7             # csrc/tok_common.h: |error in Phi| of the GELU polynomial


def row_map(route, rows, n, h, w):
    """Which partial row takes an output pixel (n x h x w, flat), or None where this module does not restate it.  The persistent
    kernels give the workgroup of row r the pixel tiles r, r + rows, r + 2 rows ... (conv_igemm.hip / pw_gemm.hip: 128 consecutive
    pixels; conv_win.hip: 256 / tw flattened rows x tw columns, x-tiles fastest); gemm256.hip writes one row per 256-pixel tile."""
    m = n * h * w
    if route == 'gemm256':
        return torch.arange(m) // 256
    if route.startswith('conv_win<'):
        tw = int(route[9:route.index(',')])
        it = (torch.arange(n * h) // (256 // tw))[:, None] * cdiv(w, tw) + (torch.arange(w) // tw)[None, :]
        return (it % rows).reshape(-1)
    if route.startswith('ring<') or (route.startswith('igemm<') and 'gather_s2' not in route):
        return (torch.arange(m) // 128) % rows
    return None          # stem window kernel, stride-2 data gradients (parity classes interleaved): the fold only


def stat_chain(rows, tile_pixels, tiles):
    """values one partial row sums: the tiles a workgroup walks (persistent grids deal tiles round robin) times the pixels of a tile"""
    return cdiv(tiles, rows) * tile_pixels


# ---- operands, references ----------------------------------------------------------------------------------------------------------
class Layer:
    """bf16-rounded operands of one layer and the fp64 references (F.conv2d / torch.nn.grad.conv2d_input) with their magnitude terms"""

    def __init__(self, geo, seed):
        n, h, w, c, k, r, stride, pad = geo
        self.geo, self.d = geo, mk(*geo)
        d = self.d
        g = torch.Generator().manual_seed(seed)
        self.x = torch.randn(n, h, w, c, generator=g).to(BF)
        wm = (torch.randn(k, r, r, c, generator=g) * (r * r * c) ** -0.5).to(BF)
        if c == 4:
            self.x[..., 3] = 0
            wm[..., 3] = 0
        self.w = wm                                                    # master [k][r][s][c]
        self.wf = torch.zeros(k, r, d.s_pad, c, dtype=BF)              # forward operand [k][r][s_pad][c]
        self.wf[:, :, :r, :] = wm
        self.wd = wm.flip(1, 2).permute(3, 1, 2, 0).contiguous()       # dgrad operand [c][r][s][k], taps flipped
        self.dy = torch.randn(n, d.p, d.q, k, generator=g).to(BF)
        self.gen = g
        self.kw = dict(stride=stride, padding=pad)
        self.m_out, self.m_in = n * d.p * d.q, n * h * w

    def randn(self, *shape):
        return torch.randn(*shape, generator=self.gen)

    def pointwise(self):
        _, _, _, _, _, r, stride, pad = self.geo
        return r == 1 and stride == 1 and pad == 0

    def fwd_ref(self):
        if self.pointwise():                               # a matmul
            x, w = self.x.double().view(-1, self.d.c), self.w.double().view(self.d.k, self.d.c).t()
            return x @ w, x.abs() @ w.abs()
        x, w = self.x.double().permute(0, 3, 1, 2), self.w.double().permute(0, 3, 1, 2)
        nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(-1, self.d.k)        # noqa: E731
        return nhwc(F.conv2d(x, w, **self.kw)), nhwc(F.conv2d(x.abs(), w.abs(), **self.kw))

    def dgrad_ref(self):
        d = self.d
        if self.pointwise():
            g, w = self.dy.double().view(-1, d.k), self.w.double().view(d.k, d.c)
            return g @ w, g.abs() @ w.abs()
        g, w = self.dy.double().permute(0, 3, 1, 2), self.w.double().permute(0, 3, 1, 2)
        shape = (d.n, d.c, d.h, d.w)
        nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(-1, d.c)              # noqa: E731
        return (nhwc(torch.nn.grad.conv2d_input(shape, w, g, **self.kw)),
                nhwc(torch.nn.grad.conv2d_input(shape, w.abs(), g.abs(), **self.kw)))

    # guards: one halo of the gathered tensor or one 128-row tile, whichever is larger (helpers.halo_guard)
    def g_x(self):
        return halo_guard(self.d.pad, self.d.w, self.d.c, self.d.c)

    def g_dy(self):
        return halo_guard(self.d.r - 1 - self.d.pad, self.d.q, self.d.k, self.d.k)


def gelu64(t):
    return t * 0.5 * (1.0 + torch.erf(t * 0.5 ** 0.5))


def gelu_d64(t):
    return 0.5 * (1.0 + torch.erf(t * 0.5 ** 0.5)) + t * torch.exp(-0.5 * t * t) * 0.3989422804014327


def check_stats(sv, rows, chain, own, own2, what, tag, pad_from=None, row_of=None):
    """sv [2][rows][c] fp32 as the kernel left it (sentinel pre-fill): every announced row written and finite; the fold of the
    rows against fp64 sums of the kernel's own stored values (`own` -> first half, `own2` -> second half) within the
    any-order summation bound 2 chain 2^-24 of the magnitudes; gemm256's pad rows (pad_from ...) exactly zero.
    With `row_of` (row_map) EVERY ROW is compared with the fp64 sums over its own pixels under the same per-row bound: a row
    holds `chain` values, so the bound is ~chain 2^-23 mean|y| while sums of the fp32 accumulators would sit
    ~2^-9 sqrt(chain) mean|y| away - for a few hundred to a thousand values per row that is 10 to 100 times the bound, so this
    is the check that tells stored values from accumulators on the long layers, where the fold alone could not."""
    assert not (sv.view(torch.int32) == 0x5A5B5C5D).any(), f'{what}: statistics rows left unwritten'
    assert torch.isfinite(sv).all(), f'{what}: non-finite statistics'
    if pad_from is not None:
        assert not sv[:, pad_from:].any(), f'{what}: padding rows behind the last pixel tile are not zero'
    if row_of is not None:
        def per_row(v):
            return torch.zeros(rows, v.shape[1], dtype=torch.float64).index_add_(0, row_of, v)
        assert_bounded(sv[0].double(), per_row(own), per_row(own.abs()), 0.0, 2 * chain * U32, f'{what} rows', tag)
        assert_bounded(sv[1].double(), per_row(own2), per_row(own2.abs()), 0.0, 2 * chain * U32, f'{what} second rows', tag)
    s = sv.double().sum(1)
    assert_bounded(s[0], own.sum(0), own.abs().sum(0), 0.0, 2 * chain * U32, f'{what} sum', tag)
    assert_bounded(s[1], own2.sum(0), own2.abs().sum(0), 0.0, 2 * chain * U32, f'{what} second sum', tag)


# ---- forward -------------------------------------------------------------------------------------------------------------------------
# (id, (n, h, w, c, k, r, stride, pad), entry, route): entry 'fwd' = tok_conv_fwd with bias and statistics (stem window: no bias),
# 'relu' / 'gelu' = tok_conv_fwd_act, 'bnep' = tok_conv_fwd_bn_apply with shortcut, mask and ReLU, 'bnep0' = without any of them
FWD_CASES = [
    # two-buffer implicit GEMM, gather mode
    ('gather64_tiny_c', (2, 8, 8, 8, 24, 3, 1, 1), 'fwd', 'igemm<128,64,gather>'),              # C < BK, K not a multiple of 64, n*p*q = 128
    ('gather64_s2_odd', (2, 15, 13, 32, 64, 3, 2, 1), 'fwd', 'igemm<128,64,gather>'),            # odd h, w under stride 2
    ('gather128_s2_ragged', (2, 17, 19, 64, 128, 3, 2, 1), 'fwd', 'igemm<128,128,gather>'),
    ('gather128_7x7_deep', (1, 7, 7, 512, 512, 3, 1, 1), 'fwd', 'igemm<128,128,gather>'),        # n = 1, 7 x 7, deepest reduction (4608)
    ('gather128_1x1_out', (70, 2, 2, 64, 128, 3, 2, 1), 'fwd', 'igemm<128,128,gather>'),         # 1 x 1 outputs: every row another image
    ('gather64_2x2_out', (40, 4, 4, 16, 64, 3, 2, 1), 'fwd', 'igemm<128,64,gather>'),            # 2 x 2 outputs, tiles span 32 images
    ('gather64_1x1_s2', (3, 14, 14, 64, 256, 1, 2, 0), 'fwd', 'igemm<128,64,gather>'),           # downsample 1x1 / stride 2
    ('patch64_2x2s2', (2, 16, 16, 96, 192, 2, 2, 0), 'fwd', 'igemm<128,64,gather>'),             # patch embed, reduction 384
    ('patch128_2x2s2', (3, 14, 14, 384, 768, 2, 2, 0), 'fwd', 'igemm<128,128,gather>'),
    # ... pointwise modes
    ('pw1_64', (2, 16, 16, 64, 128, 1, 1, 0), 'fwd', 'igemm<128,64,pw1>'),                       # smallest reduction (64)
    ('pw1_64_ragged', (3, 9, 11, 128, 72, 1, 1, 0), 'fwd', 'igemm<128,64,pw1>'),                 # 297 rows, ragged channel tile
    ('pw1_128', (1, 20, 20, 512, 264, 1, 1, 0), 'fwd', 'igemm<128,128,pw1>'),                    # ragged 128-wide channel tile
    ('pw1_128_tokens', (4, 1, 1, 2048, 1000, 1, 1, 0), 'fwd', 'igemm<128,128,pw1>'),             # linear 2048 -> 1000, 4 rows
    ('pw3_64_relu', (2, 16, 16, 64, 128, 1, 1, 0), 'relu', 'igemm<128,64,pw3>'),
    ('pw3_64_gelu', (3, 9, 11, 96, 384, 1, 1, 0), 'gelu', 'igemm<128,64,pw3>'),
    ('pw3_128_gelu', (50, 1, 1, 96, 392, 1, 1, 0), 'gelu', 'igemm<128,128,pw3>'),                # token rows: 128-wide at every depth
    ('pw3_128_relu', (1, 20, 20, 512, 256, 1, 1, 0), 'relu', 'igemm<128,128,pw3>'),
    ('pw4_full', (2, 15, 13, 64, 256, 1, 1, 0), 'bnep', 'igemm<128,64,pw4>'),                    # 390 rows: ragged last pixel tile
    ('pw4_plain', (2, 15, 13, 64, 256, 1, 1, 0), 'bnep0', 'igemm<128,64,pw4>'),
    ('pw4_deep', (1, 7, 7, 2048, 512, 1, 1, 0), 'bnep', 'igemm<128,64,pw4>'),                    # deep reduction, 49 rows
    # ... c4 stem form off and on the shared window
    ('c4_odd_width', (2, 33, 35, 4, 64, 7, 2, 3), 'fwd', 'igemm<128,64,c4>'),
    ('stem_win', (4, 70, 72, 4, 64, 7, 2, 3), 'fwd', 'stem_win'),                                # ragged tile edges (35 x 36 outputs)
    ('stem_win_k32', (3, 64, 96, 4, 32, 7, 2, 3), 'fwd', 'stem_win'),
    # pointwise ring (>= 100 000 rows, 64-wide tiles)
    ('ring_64to256', (33, 56, 56, 64, 256, 1, 1, 0), 'fwd', 'ring<64>'),                         # 103 488 rows: ragged last pixel tile
    ('ring_256to64', (32, 56, 56, 256, 64, 1, 1, 0), 'fwd', 'ring<64>'),
    ('ring_bnep', (33, 56, 56, 64, 256, 1, 1, 0), 'bnep', 'ring<64,bnep>'),
    ('ring_bnep_plain', (32, 56, 56, 256, 64, 1, 1, 0), 'bnep0', 'ring<64,bnep>'),
    ('ring_refused_act', (32, 56, 56, 64, 256, 1, 1, 0), 'relu', 'igemm<128,64,pw3>@ring_grid'),  # a mode the ring does not carry
    # 256 x 256 tiles at the default rule, and the modes gemm256 does not carry on a layer it owns
    ('g256', (8, 32, 32, 1024, 1024, 1, 1, 0), 'fwd', 'gemm256'),
    ('g256_ragged', (4, 65, 65, 512, 384, 1, 1, 0), 'fwd', 'gemm256'),                           # 16 900 rows, channel tiles 256 + 128
    ('g256_layer_bnep', (4, 65, 65, 512, 384, 1, 1, 0), 'bnep', 'igemm<128,64,pw4>@g256_layer'),
    ('g256_layer_act', (4, 65, 65, 512, 384, 1, 1, 0), 'gelu', 'igemm<128,128,pw3>@g256_layer'),
    # shared-window 3x3 kernel: every column tile x every channel tile
    ('win16_128_two_images', (5, 14, 14, 256, 256, 3, 1, 1), 'fwd', 'conv_win<16,128>'),         # a tile spans two images
    ('win16_128_ragged', (5, 13, 15, 40, 136, 3, 1, 1), 'fwd', 'conv_win<16,128>'),              # C = 40, K = 136: ragged channel tile
    ('win32_128', (3, 28, 28, 128, 128, 3, 1, 1), 'fwd', 'conv_win<32,128>'),
    ('win64_128', (2, 56, 56, 64, 128, 3, 1, 1), 'fwd', 'conv_win<64,128>'),
    ('win64_96_ragged_x', (1, 40, 72, 96, 96, 3, 1, 1), 'fwd', 'conv_win<64,96>'),               # n = 1, second x-tile ragged
    ('win32_96', (2, 16, 32, 192, 192, 3, 1, 1), 'fwd', 'conv_win<32,96>'),
    ('win16_96', (3, 12, 12, 96, 96, 3, 1, 1), 'fwd', 'conv_win<16,96>'),                        # narrowest map the kernel takes
    ('win64_64', (2, 56, 56, 64, 64, 3, 1, 1), 'fwd', 'conv_win<64,64>'),
    ('win32_64', (2, 20, 28, 32, 40, 3, 1, 1), 'fwd', 'conv_win<32,64>'),                        # smallest reduction (288), K = 40 of 64
    ('win16_64', (40, 4, 16, 64, 64, 3, 1, 1), 'fwd', 'conv_win<16,64>'),                        # 4-row images: four per tile
    ('win64_48', (1, 40, 72, 48, 48, 3, 1, 1), 'fwd', 'conv_win<64,48>'),
    ('win32_48', (2, 30, 26, 96, 48, 3, 1, 1), 'fwd', 'conv_win<32,48>'),
    ('win16_48', (3, 9, 16, 48, 48, 3, 1, 1), 'fwd', 'conv_win<16,48>'),
    ('win64_48_large', (8, 128, 128, 48, 48, 3, 1, 1), 'fwd', 'conv_win<64,48>'),                # 2048 tiles: the persistent grid walks
]


def _entry_flags(entry):
    return dict(act=entry in ('relu', 'gelu'), bnep=entry.startswith('bnep'))


def test_every_forward_route_has_a_case():
    assert {c[3] for c in FWD_CASES} == ROUTES_FWD


@pytest.mark.parametrize('case', FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_conv_fwd_contract(case):
    name, geo, entry, route = case
    lib, st = _C.lib(), stream_ptr()
    L = Layer(geo, seed=sum(geo) + len(name))
    d, tag = L.d, f'conv_contract/fwd/{name}'
    k, m = d.k, L.m_out
    on_stem_window = route == 'stem_win'
    flags = _entry_flags(entry)
    restated, rows, tile_px, tiles = route_fwd(d, bias=not on_stem_window, **flags)
    assert restated == route
    assert lib.tok_conv_fwd_stat_rows(ctypes.byref(d)) == rows

    ktot = d.r * d.s_pad * d.c
    xg, wg = gin(L.x, L.g_x()), gin(L.wf, 128 * ktot)
    bias = None if on_stem_window else L.randn(k) * 0.5
    bg = None if bias is None else gin(bias, 128)
    bp = None if bg is None else bg.ptr
    ref, mag = L.fwd_ref()
    if bias is not None and not flags['bnep']:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    depth = ktot + 1                                        # the reduction, + bias
    outs, ins = [], [(xg, 'x'), (wg, 'w')] + ([(bg, 'bias')] if bg else [])

    def fresh_y():
        y = gout(m * k, BF, 128 * k)
        outs.append((y, 'y'))
        return y

    if entry == 'fwd':
        ys = [fresh_y() for _ in range(3)]
        sts = [gout(2 * rows * k, F32, 128 * k) for _ in range(2)]
        outs += [(s, 'stats') for s in sts]
        _C.check(lib.tok_conv_fwd(ctypes.byref(d), xg.ptr, wg.ptr, bp, ys[0].ptr, sts[0].ptr, st), 'fwd')
        _C.check(lib.tok_conv_fwd(ctypes.byref(d), xg.ptr, wg.ptr, bp, ys[1].ptr, None, st), 'fwd(no stats)')
        _C.check(lib.tok_conv_fwd(ctypes.byref(d), xg.ptr, wg.ptr, bp, ys[2].ptr, sts[1].ptr, st), 'fwd(again)')
        torch.cuda.synchronize()
        y = ys[0].value().view(m, k)
        assert_bounded(y, ref, mag, A_BF, depth * U32, 'y', tag)
        assert torch.equal(ys[1].value(), ys[0].value()), 'y depends on whether statistics are requested'
        assert torch.equal(ys[2].value(), ys[0].value()) and torch.equal(sts[1].value(), sts[0].value()), 'not bit-reproducible'
        used = min(512, d.n * cdiv(d.p, 16) * cdiv(d.q, 16), rows) if on_stem_window else rows
        chain = stat_chain(used, 256, d.n * cdiv(d.p, 16) * cdiv(d.q, 16)) if on_stem_window else stat_chain(rows, tile_px, tiles)
        y64 = y.double()
        check_stats(sts[0].value().view(2, rows, k), rows, chain, y64, y64 * y64, 'fwd stats', tag,
                    pad_from=cdiv(m, 256) if route == 'gemm256' else None, row_of=row_map(route, rows, d.n, d.p, d.q))
    elif entry in ('relu', 'gelu'):
        kind = int(entry == 'gelu')
        ys, acts = [fresh_y() for _ in range(2)], [gout(m * k, BF, 128 * k) for _ in range(2)]
        outs += [(a, 'y_act') for a in acts]
        for y_, a_ in zip(ys, acts):
            _C.check(lib.tok_conv_fwd_act(ctypes.byref(d), xg.ptr, wg.ptr, bp, y_.ptr, a_.ptr, kind, st), 'fwd_act')
        torch.cuda.synchronize()
        y = ys[0].value().view(m, k)
        assert_bounded(y, ref, mag, A_BF, depth * U32, 'y', tag)
        assert torch.equal(ys[1].value(), ys[0].value()) and torch.equal(acts[1].value(), acts[0].value()), 'not bit-reproducible'
        # the activation of the bf16-ROUNDED GEMM result (include/tok.h): ReLU is exact; GELU(y) = y Phi(y) carries the
        # polynomial's error in Phi and two fp32 roundings, relative to |y|, and one bf16 rounding of the result
        y64 = y.double()
        if kind == 0:
            assert torch.equal(acts[0].value().view(m, k), torch.relu(y)), 'y_act != relu(y)'
        else:
            assert_bounded(acts[0].value().view(m, k), gelu64(y64), y64.abs(), A_BF, GELU_PHI + 2 * U32, 'y_act', tag)
    else:
        full = entry == 'bnep'
        scale, shift = 0.5 + torch.rand(k, generator=L.gen), L.randn(k) * 0.5
        short = L.randn(m, k).to(BF) if full else None
        sg, hg = gin(scale, 128), gin(shift, 128)
        og = gin(short, 128 * k) if full else None
        ins += [(sg, 'scale'), (hg, 'shift')] + ([(og, 'shortcut')] if full else [])
        ys = [fresh_y() for _ in range(2)]
        masks = [gout(m * k // 8, U8, 128 * k // 8) for _ in range(2)] if full else [None, None]
        outs += [(mk_, 'mask') for mk_ in masks if mk_ is not None]
        for y_, m_ in zip(ys, masks):
            _C.check(lib.tok_conv_fwd_bn_apply(ctypes.byref(d), xg.ptr, wg.ptr, sg.ptr, hg.ptr, og.ptr if full else None, int(full),
                                               y_.ptr, m_.ptr if full else None, st), 'fwd_bn_apply')
        torch.cuda.synchronize()
        # out = act(acc * scale + shift (+ shortcut)): the reduction, one fma, one addition
        conv, cmag = L.fwd_ref()
        pre = conv * scale.double() + shift.double() + (short.double() if full else 0.0)
        pmag = cmag * scale.double().abs() + shift.double().abs() + (short.double().abs() if full else 0.0)
        want = torch.relu(pre) if full else pre
        b = (ktot + 2) * U32
        y = ys[0].value().view(m, k)
        assert_bounded(y, want, pmag, A_BF, b, 'out', tag)
        assert torch.equal(ys[1].value(), ys[0].value()), 'not bit-reproducible'
        if full:
            # mask bit = (out > 0), bit-exact wherever the bound decides the sign of the fp64 value
            bits = unpack_bits(masks[0].value(), m, k)
            assert torch.equal(masks[1].value(), masks[0].value())
            assert torch.equal(bits, y > 0), 'mask bits are not (out > 0) of the stored tensor'
            undecided = pre.abs() <= A_BF * pre.abs() + b * pmag            # the whole bound of `out`
            assert float(undecided.double().mean()) <= 0.01
            assert torch.equal(bits[~undecided], (pre > 0)[~undecided]), 'mask bits differ from the fp64 sign'
    for buf, what in outs + ins:
        buf.check(f'{name}: {what}')


# ---- data gradient -----------------------------------------------------------------------------------------------------------------
# (id, geometry, route, extra entries beside the ones every route carries): every case runs tok_conv_dgrad with accumulate 0
# (twice: bit-reproducible), 1 onto zeros (same bits) and 1 onto data, tok_conv_dgrad_bnstats with a mask, tok_conv_dgrad_maskstore
# with +=, tok_conv_dgrad_bias with +=, BatchNorm sums and no mask
DGRAD_CASES = [
    ('gather64_s1_tiny_c', (2, 8, 8, 8, 24, 3, 1, 1), 'igemm<128,64,gather_s1>', ()),
    ('gather128_s1_7x7', (1, 7, 7, 512, 512, 3, 1, 1), 'igemm<128,128,gather_s1>', ()),          # W < 12: off the window kernel
    ('gather128_s1_k72', (2, 16, 16, 72, 64, 3, 1, 1), 'igemm<128,128,gather_s1>', ()),           # 65 ... 95 output channels of dX
    ('gather64_s2_odd', (2, 17, 19, 64, 128, 3, 2, 1), 'igemm<128,64,gather_s2>', ()),         # odd extents
    ('gather64_s2_narrow', (2, 16, 16, 64, 64, 3, 2, 1), 'igemm<128,64,gather_s2>', ()),         # 8 x 8 class maps: W < 12
    ('gather64_s2_thin', (2, 32, 32, 16, 64, 3, 2, 1), 'igemm<128,64,gather_s2>', ()),           # 16 channels < 32
    ('gather128_s2_k72', (2, 32, 32, 72, 64, 3, 2, 1), 'igemm<128,128,gather_s2>', ()),          # 72 channels: 65 ... 95
    ('gather_s2_1x1_out', (70, 2, 2, 64, 128, 3, 2, 1), 'igemm<128,64,gather_s2>', ()),
    ('gather_s2_patch', (2, 16, 16, 96, 192, 2, 2, 0), 'igemm<128,128,gather_s2>', ()),          # 2x2 / stride 2
    ('gather_s2_1x1', (3, 14, 14, 64, 256, 1, 2, 0), 'igemm<128,64,gather_s2>', ()),
    ('pw1_64', (2, 16, 16, 64, 128, 1, 1, 0), 'igemm<128,64,pw1>', ('relu', 'gelu')),
    ('pw1_128', (3, 9, 11, 264, 512, 1, 1, 0), 'igemm<128,128,pw1>', ('relu', 'gelu')),          # 297 rows, ragged channel tile
    ('pw1_tokens', (4, 1, 1, 2048, 1000, 1, 1, 0), 'igemm<128,128,pw1>', ()),
    ('win16_128_two_images', (5, 14, 14, 256, 256, 3, 1, 1), 'conv_win<16,128>', ()),
    ('win32_128', (3, 28, 28, 128, 128, 3, 1, 1), 'conv_win<32,128>', ()),
    ('win64_96_ragged_x', (1, 40, 72, 96, 96, 3, 1, 1), 'conv_win<64,96>', ()),
    ('win64_64', (2, 56, 56, 64, 64, 3, 1, 1), 'conv_win<64,64>', ()),
    ('win64_48', (1, 40, 72, 48, 48, 3, 1, 1), 'conv_win<64,48>', ()),
    ('win16_128_ragged', (5, 13, 15, 136, 40, 3, 1, 1), 'conv_win<16,128>', ()),
    ('win16_48', (3, 9, 16, 48, 48, 3, 1, 1), 'conv_win<16,48>', ()),
    ('win16_64', (40, 4, 16, 64, 64, 3, 1, 1), 'conv_win<16,64>', ()),                           # four images per tile
    ('win16_96', (3, 12, 12, 96, 96, 3, 1, 1), 'conv_win<16,96>', ()),
    ('win32_48', (2, 30, 26, 48, 96, 3, 1, 1), 'conv_win<32,48>', ()),
    ('win32_64', (2, 20, 28, 40, 32, 3, 1, 1), 'conv_win<32,64>', ()),                           # 40 of 64 channels, smallest reduction
    ('win32_96', (2, 16, 32, 192, 192, 3, 1, 1), 'conv_win<32,96>', ()),
    ('win64_128', (2, 56, 56, 128, 64, 3, 1, 1), 'conv_win<64,128>', ()),
    ('win64_48_large', (8, 128, 128, 48, 48, 3, 1, 1), 'conv_win<64,48>', ()),                   # 2048 tiles, two x-tiles per row group
    ('s2d32_128', (3, 56, 56, 128, 128, 3, 2, 1), 'conv_s2d<32,128>', ()),
    ('s2d16_128_two_images', (5, 28, 28, 256, 256, 3, 2, 1), 'conv_s2d<16,128>', ()),
    ('s2d64_48', (1, 64, 256, 48, 48, 3, 2, 1), 'conv_s2d<64,48>', ()),
    ('s2d64_96', (2, 32, 128, 96, 192, 3, 2, 1), 'conv_s2d<64,96>', ()),
    ('s2d32_96', (2, 32, 64, 192, 192, 3, 2, 1), 'conv_s2d<32,96>', ()),
    ('s2d32_64_ragged', (3, 36, 44, 64, 40, 3, 2, 1), 'conv_s2d<32,64>', ()),                    # 18 x 22 class maps, 40 gathered channels
    ('s2d16_48', (2, 24, 32, 48, 48, 3, 2, 1), 'conv_s2d<16,48>', ()),
    ('s2d16_64', (2, 24, 28, 64, 64, 3, 2, 1), 'conv_s2d<16,64>', ()),
    ('s2d16_96', (2, 24, 24, 96, 96, 3, 2, 1), 'conv_s2d<16,96>', ()),                           # 12-wide class maps: the narrowest served
    ('s2d32_48', (2, 40, 56, 48, 96, 3, 2, 1), 'conv_s2d<32,48>', ()),
    ('s2d64_64', (1, 32, 80, 64, 40, 3, 2, 1), 'conv_s2d<64,64>', ()),                           # n = 1
    ('s2d64_128', (1, 32, 96, 128, 64, 3, 2, 1), 'conv_s2d<64,128>', ()),
    ('ring_256to64', (32, 56, 56, 64, 256, 1, 1, 0), 'ring<64>', ('subacc', 'dgrad2', 'relu')),   # dX 64 wide from 256
    ('ring_64to256', (33, 56, 56, 256, 64, 1, 1, 0), 'ring<64>', ()),                            # ragged last pixel tile
    ('g256', (8, 32, 32, 1024, 1024, 1, 1, 0), 'gemm256', ('gelu',)),
    ('g256_ragged', (4, 65, 65, 384, 512, 1, 1, 0), 'gemm256', ()),
]


def test_every_dgrad_route_has_a_case():
    assert {c[2] for c in DGRAD_CASES} == ROUTES_DGRAD
    assert {'subacc', 'dgrad2', 'relu', 'gelu'} <= {e for c in DGRAD_CASES for e in c[3]}


@pytest.mark.parametrize('case', DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
def test_conv_dgrad_contract(case):
    name, geo, route, extra = case
    lib, st = _C.lib(), stream_ptr()
    L = Layer(geo, seed=7 * sum(geo) + len(name))
    d, tag = L.d, f'conv_contract/dgrad/{name}'
    c, m = d.c, L.m_in
    restated, rows, tile_px, tiles = route_dgrad(d)
    assert restated == route
    assert lib.tok_conv_dgrad_stat_rows(ctypes.byref(d)) == rows
    chain = stat_chain(rows, tile_px, tiles)
    pad_from = cdiv(m, 256) if route == 'gemm256' else None
    ktot = d.r * d.s * d.k
    gg, wg = gin(L.dy, L.g_dy()), gin(L.wd, 128 * ktot)
    ref, mag = L.dgrad_ref()
    old = L.randn(m, c).to(BF)
    bn_y = L.randn(m, c).to(BF)
    bits = torch.rand(m, c, generator=L.gen) < 0.6
    bias = L.randn(c) * 0.5
    yg, mg, bg = gin(bn_y, 128 * c), gin(pack_bits(bits), 128 * c // 8), gin(bias, 128)
    outs, ins = [], [(gg, 'dy'), (wg, 'w_dgrad'), (yg, 'bn_y'), (mg, 'mask'), (bg, 'bias')]
    D = ctypes.byref(d)

    def dx_buf(init=None):
        b = gout(m * c, BF, halo_guard(d.pad, d.w, c, c), init=init)
        outs.append((b, 'dx'))
        return b

    def part_buf():
        b = gout(2 * rows * c, F32, 128 * c)
        outs.append((b, 'partial'))
        return b

    # plain: =, = again, += onto zeros, += onto data
    p0, p1, pz, pa = dx_buf(), dx_buf(), dx_buf(torch.zeros(m, c, dtype=BF)), dx_buf(old)
    for buf, acc in ((p0, 0), (p1, 0), (pz, 1), (pa, 1)):
        _C.check(lib.tok_conv_dgrad(D, gg.ptr, wg.ptr, buf.ptr, acc, st), 'dgrad')
    # BatchNorm-backward sums with a mask; masked store with +=; bias with += and sums without a mask
    # (every epilogue call runs twice into fresh buffers: dx AND the partial rows bit-reproducible)
    twice = []

    def again(first, second, what):
        twice.append((first, second, what))
        return first

    def same_bits():
        torch.cuda.synchronize()
        for first, second, what in twice:
            assert torch.equal(first.value(), second.value()), f'{what}: not bit-reproducible'
        del twice[:]

    for rep_ in range(2):
        s_dx, s_part = dx_buf(), part_buf()
        _C.check(lib.tok_conv_dgrad_bnstats(D, gg.ptr, wg.ptr, s_dx.ptr, 0, yg.ptr, mg.ptr, s_part.ptr, st), 'dgrad_bnstats')
        m_dx, m_part = dx_buf(old), part_buf()
        _C.check(lib.tok_conv_dgrad_maskstore(D, gg.ptr, wg.ptr, m_dx.ptr, 1, mg.ptr, m_part.ptr, st), 'dgrad_maskstore')
        b_dx, b_part = dx_buf(old), part_buf()
        _C.check(lib.tok_conv_dgrad_bias(D, gg.ptr, wg.ptr, bg.ptr, b_dx.ptr, 1, yg.ptr, None, b_part.ptr, st), 'dgrad_bias')
        if rep_ == 0:
            firsts = (s_dx, s_part, m_dx, m_part, b_dx, b_part)
        else:
            for f_, s_, w_ in zip(firsts, (s_dx, s_part, m_dx, m_part, b_dx, b_part),
                                  ('bnstats dx', 'bnstats partial', 'maskstore dx', 'maskstore partial', 'bias dx', 'bias partial')):
                again(f_, s_, w_)
    same_bits()
    row_of = row_map(route, rows, d.n, d.h, d.w)

    o64, y64, bit64 = old.double(), bn_y.double(), bits.double()
    v0 = p0.value().view(m, c)
    assert_bounded(v0, ref, mag, A_BF, ktot * U32, 'dx', tag)
    assert torch.equal(p1.value(), p0.value()), 'not bit-reproducible'
    assert torch.equal(pz.value(), p0.value()), '+= onto zeros differs from ='
    assert_bounded(pa.value().view(m, c), o64 + ref, o64.abs() + mag, A_BF, (ktot + 1) * U32, 'dx +=', tag)
    # bnstats: dx as the plain call stores it; sums of dz = mask ? dx : 0 and dz * bn_y over the STORED dx
    assert torch.equal(s_dx.value(), p0.value()), 'dx depends on the statistics request'
    dz = v0.double() * bit64
    check_stats(s_part.value().view(2, rows, c), rows, chain, dz, dz * y64, 'bnstats partial', tag, pad_from, row_of)
    # maskstore: zeros where the bit is clear, the += result elsewhere; first half sum(dz), second half zero
    mv = m_dx.value().view(m, c)
    assert not mv[~bits].any(), 'masked positions are not stored as zeros'
    assert_bounded(mv, (o64 + ref) * bit64, (o64.abs() + mag) * bit64, A_BF, (ktot + 1) * U32, 'dz (mask store)', tag)
    mp = m_part.value().view(2, rows, c)
    assert not mp[1].any(), 'second half of the mask-store partial rows is not zero'
    mv64 = mv.double()
    check_stats(mp, rows, chain, mv64, mv64 * 0, 'maskstore partial', tag, pad_from, row_of)
    # bias: reduction + bias + old value
    b64 = bias.double()
    bv = b_dx.value().view(m, c)
    assert_bounded(bv, o64 + ref + b64, o64.abs() + mag + b64.abs(), A_BF, (ktot + 2) * U32, 'dx (bias, +=)', tag)
    bv64 = bv.double()
    check_stats(b_part.value().view(2, rows, c), rows, chain, bv64, bv64 * y64, 'bias partial', tag, pad_from, row_of)

    for kind_name in [e for e in extra if e in ('relu', 'gelu')]:
        # dx = bf16(bf16(GEMM) * act'(act_x)): against the fp64 derivative times the plain call's stored result.  ReLU's factor
        # is exact; GELU's Phi + x phi carries the polynomial's error in Phi, one v_exp_f32 and three fp32 roundings (<= 8 ulp of 1)
        kind = int(kind_name == 'gelu')
        assert route_dgrad(d, act=True).name == ACT_ROUTES[name]
        ax = L.randn(m, c).to(BF)
        ag, a_dx, a_dx2 = gin(ax, 128 * c), dx_buf(), dx_buf()
        ins.append((ag, 'act_x'))
        _C.check(lib.tok_conv_dgrad_act(D, gg.ptr, wg.ptr, ag.ptr, kind, a_dx.ptr, st), 'dgrad_act')
        _C.check(lib.tok_conv_dgrad_act(D, gg.ptr, wg.ptr, ag.ptr, kind, a_dx2.ptr, st), 'dgrad_act')
        again(a_dx, a_dx2, f'dx ({kind_name})')
        same_bits()
        fac = (ax.double() > 0).double() if kind == 0 else gelu_d64(ax.double())
        eps = 0.0 if kind == 0 else GELU_PHI + 8 * U32
        av = a_dx.value().view(m, c)
        # against fp64 throughout: two bf16 roundings (2 A + A^2) of the product; the accumulation error and the first rounding
        # scaled by |act'| <= 1.13 (its maximum, at x = sqrt 2); the derivative's own error relative to the magnitude
        assert_bounded(av, ref * fac, mag, 2 * A_BF + A_BF * A_BF, 1.13 * (1 + A_BF) * ktot * U32 + (1 + A_BF) * eps,
                       f'dx ({kind_name}) vs fp64', tag)
        if route.startswith('igemm'):
            # the plain call ran the same kernel: its stored result IS the rounded GEMM result, one bf16 rounding remains.
            # (On a ring or gemm256 layer the plain call runs ANOTHER kernel than the fused one - the two-buffer kernel in PW 3
            #  mode takes over - whose fp32 sums may round to a neighbouring bf16 value: the rounded GEMM result of the fused
            #  launch is not observable there, so only the fp64 check above applies.)
            assert_bounded(av, v0.double() * fac, v0.double().abs(), A_BF, eps, f'dx ({kind_name})', tag)

    if 'subacc' in extra:
        assert lib.tok_conv_dgrad_subacc_ok(D) == 1 and route_dgrad(d, sub=True).name == 'ring<64>'
        h2, w2 = cdiv(d.h, 2), cdiv(d.w, 2)
        dsub = L.randn(d.n, h2, w2, c).to(BF)
        sg, u_dx, u_part = gin(dsub, 128 * c), dx_buf(), part_buf()
        ins.append((sg, 'dsub'))
        _C.check(lib.tok_conv_dgrad_subacc(D, gg.ptr, wg.ptr, u_dx.ptr, sg.ptr, yg.ptr, mg.ptr, u_part.ptr, 0, st), 'dgrad_subacc')
        w_dx, w_part = dx_buf(), part_buf()
        _C.check(lib.tok_conv_dgrad_subacc(D, gg.ptr, wg.ptr, w_dx.ptr, sg.ptr, None, mg.ptr, w_part.ptr, 1, st), 'dgrad_subacc(mask)')
        u2_dx, u2_part, w2_dx, w2_part = dx_buf(), part_buf(), dx_buf(), part_buf()
        _C.check(lib.tok_conv_dgrad_subacc(D, gg.ptr, wg.ptr, u2_dx.ptr, sg.ptr, yg.ptr, mg.ptr, u2_part.ptr, 0, st), 'dgrad_subacc')
        _C.check(lib.tok_conv_dgrad_subacc(D, gg.ptr, wg.ptr, w2_dx.ptr, sg.ptr, None, mg.ptr, w2_part.ptr, 1, st), 'dgrad_subacc(mask)')
        for f_, s_, w_ in ((u_dx, u2_dx, 'subacc dx'), (u_part, u2_part, 'subacc partial'), (w_dx, w2_dx, 'subacc mask dx'),
                           (w_part, w2_part, 'subacc mask partial')):
            again(f_, s_, w_)
        same_bits()
        scat = torch.zeros(d.n, d.h, d.w, c, dtype=torch.float64)
        scat[:, ::2, ::2] = dsub.double()
        scat = scat.view(m, c)
        uv = u_dx.value().view(m, c)
        assert_bounded(uv, ref + scat, mag + scat.abs(), A_BF, (ktot + 1) * U32, 'dx (subacc)', tag)
        udz = uv.double() * bit64
        check_stats(u_part.value().view(2, rows, c), rows, chain, udz, udz * y64, 'subacc partial', tag, None, row_of)
        wv = w_dx.value().view(m, c)
        assert not wv[~bits].any()
        assert_bounded(wv, (ref + scat) * bit64, (mag + scat.abs()) * bit64, A_BF, (ktot + 1) * U32, 'dz (subacc, mask store)', tag)
        check_stats(w_part.value().view(2, rows, c), rows, chain, wv.double(), wv.double() * 0, 'subacc mask partial', tag, None, row_of)

    if 'dgrad2' in extra:
        # dx += dgrad(d; dy, w) + dgrad(d2; dy2, w2) + bias: both reductions, the bias, the old value
        L2 = Layer((d.n, d.h, d.w, c, 64, 1, 1, 0), seed=99)
        d2 = L2.d
        assert lib.tok_conv_dgrad2_ok(D, ctypes.byref(d2)) == 1
        assert pick_bn(d2.c, d2.k) == 64 and pw_serves(64, m, d.k, c) and pw_serves(64, m, d2.k, c)
        rows2 = lib.tok_conv_dgrad_stat_rows(ctypes.byref(d2))
        assert rows2 == route_dgrad(d2).rows
        g2, w2g = gin(L2.dy, 128 * d2.k), gin(L2.wd, 128 * d2.k)
        ins += [(g2, 'dy2'), (w2g, 'w2_dgrad')]
        t_dx, t_part = dx_buf(old), gout(2 * rows2 * c, F32, 128 * c)
        outs.append((t_part, 'partial (dgrad2)'))
        _C.check(lib.tok_conv_dgrad2(D, gg.ptr, wg.ptr, ctypes.byref(d2), g2.ptr, w2g.ptr, bg.ptr, t_dx.ptr, 1, yg.ptr, mg.ptr,
                                     t_part.ptr, st), 'dgrad2')
        t2_dx, t2_part = dx_buf(old), gout(2 * rows2 * c, F32, 128 * c)
        outs.append((t2_part, 'partial (dgrad2)'))
        _C.check(lib.tok_conv_dgrad2(D, gg.ptr, wg.ptr, ctypes.byref(d2), g2.ptr, w2g.ptr, bg.ptr, t2_dx.ptr, 1, yg.ptr, mg.ptr,
                                     t2_part.ptr, st), 'dgrad2')
        again(t_dx, t2_dx, 'dgrad2 dx')
        again(t_part, t2_part, 'dgrad2 partial')
        same_bits()
        ref2, mag2 = L2.dgrad_ref()
        tv = t_dx.value().view(m, c)
        assert_bounded(tv, o64 + ref + ref2 + b64, o64.abs() + mag + mag2 + b64.abs(), A_BF, (ktot + d2.k + 2) * U32,
                       'dx (dgrad2)', tag)
        tdz = tv.double() * bit64
        check_stats(t_part.value().view(2, rows2, c), rows2, stat_chain(rows2, 128, cdiv(m, 128)), tdz, tdz * y64,
                    'dgrad2 partial', tag, None, row_map('ring<64>', rows2, d.n, d.h, d.w))

    for buf, what in outs + ins:
        buf.check(f'{name}: {what}')


# ---- refusals: TOK_ERR_INVALID / the entry named in the message / nothing written ------------------------------------------------
def _refused(rc, msg, outs, code=ERR_INVALID):
    err = last_error()
    assert rc == code, (rc, err)
    assert msg in err, (msg, err)
    torch.cuda.synchronize()
    for o in outs:
        assert o.untouched(), f'a refused call ({msg}) wrote to an output'
        o.check(msg)


def _desc(**kw):
    base = dict(n=2, h=16, w=16, c=64, k=64, r=3, s=3, p=16, q=16, stride=1, pad=1, s_pad=3)
    base.update(kw)
    return _C.ConvDesc(*(base[f] for f in 'n h w c k r s p q stride pad s_pad'.split()))


BAD_DESCS = [None, dict(n=0), dict(h=0), dict(w=0), dict(c=0), dict(k=0), dict(r=0), dict(s=0), dict(r=0, s=0), dict(stride=0),
             dict(pad=-1), dict(k=60), dict(c=60), dict(p=15), dict(q=17),
             dict(s_pad=8), dict(c=4, s_pad=3), dict(n=1 << 24, h=16, w=16)]


def test_conv_refusals():
    lib, st = _C.lib(), stream_ptr()
    n_el = 2 * 16 * 16 * 64
    src = gin(torch.zeros(n_el, dtype=BF), 1024)
    wsrc = gin(torch.zeros(64 * 9 * 64, dtype=BF), 1024)
    fsrc = gin(torch.zeros(4096, dtype=F32), 1024)
    msrc = gin(torch.zeros(n_el // 8, dtype=U8), 1024)
    out, out2 = gout(n_el, BF, 1024), gout(n_el, BF, 1024)
    part = gout(2 * 64 * 64, F32, 1024)
    mask = gout(n_el // 8, U8, 1024)
    O = [out, out2, part, mask]
    for bad in BAD_DESCS:
        D = None if bad is None else ctypes.byref(_desc(**bad))        # (None: a null descriptor)
        _refused(lib.tok_conv_fwd(D, src.ptr, wsrc.ptr, None, out.ptr, part.ptr, st), 'tok_conv_fwd', O)
        _refused(lib.tok_conv_dgrad(D, src.ptr, wsrc.ptr, out.ptr, 0, st), 'tok_conv_dgrad', O)
        _refused(lib.tok_conv_dgrad_bnstats(D, src.ptr, wsrc.ptr, out.ptr, 0, src.ptr, None, part.ptr, st), 'tok_conv_dgrad_bnstats', O)
        assert lib.tok_conv_fwd_stat_rows(D) == ERR_INVALID and lib.tok_conv_dgrad_stat_rows(D) == ERR_INVALID
        assert lib.tok_conv_dgrad_subacc_ok(D) == 0
    # the data gradient: no c4 input, pad <= r - 1, square filters
    c4 = mk(2, 32, 32, 4, 64, 7, 2, 3)
    _refused(lib.tok_conv_dgrad(ctypes.byref(c4), src.ptr, wsrc.ptr, out.ptr, 0, st), 'tok_conv_dgrad: c4', O)
    wide = _desc(r=1, s=1, s_pad=1, pad=1, p=18, q=18)
    _refused(lib.tok_conv_dgrad(ctypes.byref(wide), src.ptr, wsrc.ptr, out.ptr, 0, st), 'tok_conv_dgrad: pad > r-1', O)
    flat = _desc(r=3, s=1, s_pad=1, pad=0, p=14, q=16)
    _refused(lib.tok_conv_dgrad(ctypes.byref(flat), src.ptr, wsrc.ptr, out.ptr, 0, st), 'tok_conv_dgrad: square filters only', O)
    # fused epilogues on a 3x3 layer
    d3 = _desc()
    D3 = ctypes.byref(d3)
    _refused(lib.tok_conv_fwd_act(D3, src.ptr, wsrc.ptr, None, out.ptr, out2.ptr, 0, st), 'tok_conv_fwd_act: 1x1', O)
    _refused(lib.tok_conv_dgrad_act(D3, src.ptr, wsrc.ptr, src.ptr, 1, out.ptr, st), 'tok_conv_dgrad_act: 1x1', O)
    _refused(lib.tok_conv_fwd_bn_apply(D3, src.ptr, wsrc.ptr, fsrc.ptr, fsrc.ptr, None, 1, out.ptr, mask.ptr, st),
             'tok_conv_fwd_bn_apply', O)
    _refused(lib.tok_conv_fwd_act(D3, src.ptr, wsrc.ptr, None, out.ptr, out2.ptr, 2, st), 'tok_conv_fwd_act', O)
    # subacc / dgrad2 off the ring (a pointwise layer of 512 rows)
    d1 = _desc(r=1, s=1, s_pad=1, pad=0)
    D1 = ctypes.byref(d1)
    assert lib.tok_conv_dgrad_subacc_ok(D1) == 0 and lib.tok_conv_dgrad2_ok(D1, D1) == 0
    _refused(lib.tok_conv_dgrad_subacc(D1, src.ptr, wsrc.ptr, out.ptr, src.ptr, None, None, None, 0, st), 'tok_conv_dgrad_subacc', O)
    _refused(lib.tok_conv_dgrad_subacc(D3, src.ptr, wsrc.ptr, out.ptr, src.ptr, None, None, None, 0, st), 'tok_conv_dgrad_subacc: 1x1', O)
    _refused(lib.tok_conv_dgrad2(D1, src.ptr, wsrc.ptr, D1, src.ptr, wsrc.ptr, None, out.ptr, 0, None, None, None, st),
             'tok_conv_dgrad2', O)
    # arguments that go together
    _refused(lib.tok_conv_dgrad_bnstats(D1, src.ptr, wsrc.ptr, out.ptr, 0, None, None, part.ptr, st), 'tok_conv_dgrad_bnstats', O)
    _refused(lib.tok_conv_dgrad_maskstore(D1, src.ptr, wsrc.ptr, out.ptr, 0, None, part.ptr, st), 'tok_conv_dgrad_maskstore', O)
    _refused(lib.tok_conv_dgrad_bias(D1, src.ptr, wsrc.ptr, fsrc.ptr, out.ptr, 0, src.ptr, None, None, st), 'tok_conv_dgrad_bias', O)
    _refused(lib.tok_conv_fwd(D1, None, wsrc.ptr, None, out.ptr, None, st), 'tok_conv_fwd: null pointer', O)
    _refused(lib.tok_conv_dgrad(D1, src.ptr, None, out.ptr, 0, st), 'tok_conv_dgrad: null pointer', O)
    for b in (src, wsrc, fsrc, msrc):
        b.check('input')


# ---- tok_relu_mask_reduce: the stand-alone form of the masked store (csrc/unit3.hip) ---------------------------------------------
# (300, 2176): two channel-group passes per lane, the second one ragged (16 of 256 lanes live)
@pytest.mark.parametrize('m,c', [(1, 8), (777, 48), (4096 + 17, 256), (50176, 64), (300, 2048), (300, 2176)])
@pytest.mark.parametrize('mode', ['mask', 'in_place', 'no_mask'])
def test_relu_mask_reduce_contract(m, c, mode):
    """dz = mask ? dout : 0 exactly (bf16 in, bf16 out); partial[2][tok_bn_bwd_rows(m, c)][c]: the first half folds to the column
    sums of the stored dz, the second half is zero, every row written.  A row sums at most ceil(m / rows) values per lane chain
    plus the 256 lanes folded in order: bound 2 (ceil(m / rows) + 256) 2^-24 of the magnitudes."""
    lib, st = _C.lib(), stream_ptr()
    g = torch.Generator().manual_seed(m + c)
    dout = torch.randn(m, c, generator=g).to(BF)
    bits = torch.rand(m, c, generator=g) < 0.5
    rows = lib.tok_bn_bwd_rows(m, c)
    assert rows > 0
    outs = []
    for _ in range(2):
        src = gout(m * c, BF, 128 * c, init=dout) if mode == 'in_place' else gin(dout, 128 * c)
        mg = None if mode == 'no_mask' else gin(pack_bits(bits), 128 * c // 8)
        dz = src if mode == 'in_place' else gout(m * c, BF, 128 * c)
        part = gout(2 * rows * c, F32, 128 * c)
        _C.check(lib.tok_relu_mask_reduce(src.ptr, None if mg is None else mg.ptr, m, c, dz.ptr, part.ptr, st), 'relu_mask_reduce')
        outs.append((src, mg, dz, part))
    torch.cuda.synchronize()
    for src, mg, dz, part in outs:
        for b in (src, dz, part) + (() if mg is None else (mg,)):
            b.check(mode)
    (_, _, dz, part), (_, _, dz2, part2) = outs
    assert torch.equal(dz.value(), dz2.value()) and torch.equal(part.value(), part2.value()), 'not bit-reproducible'
    want = dout if mode == 'no_mask' else torch.where(bits, dout, torch.zeros_like(dout))
    assert torch.equal(dz.value().view(m, c), want), 'dz != mask ? dout : 0'
    w64 = want.double()
    check_stats(part.value().view(2, rows, c), rows, cdiv(m, rows) + 256, w64, w64 * 0, 'relu_mask_reduce partial',
                f'conv_contract/relu_mask_reduce/{mode}_m{m}_c{c}')
    assert not part.value().view(2, rows, c)[1].any()


def test_relu_mask_reduce_refusals():
    lib, st = _C.lib(), stream_ptr()
    src = gin(torch.zeros(64 * 16, dtype=BF), 1024)
    dz, part = gout(64 * 16, BF, 1024), gout(2 * 64 * 16, F32, 1024)
    for args in ((None, None, 64, 16, dz.ptr, part.ptr), (src.ptr, None, 64, 16, None, part.ptr), (src.ptr, None, 64, 16, dz.ptr, None),
                 (src.ptr, None, 0, 16, dz.ptr, part.ptr), (src.ptr, None, 64, 12, dz.ptr, part.ptr)):
        _refused(lib.tok_relu_mask_reduce(*args, st), 'tok_relu_mask_reduce', [dz, part])
