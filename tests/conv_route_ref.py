"""The routes of the convolution forward and data gradient (route_fwd / route_dgrad of csrc/conv_igemm.hip, made of the predicates of
conv_win.hip, conv_s2d.hip, gemm256.hip, stem.hip and pw_gemm.hip), restated: which kernel runs a layer under a mode and how many
partial-statistics rows it writes.  One function per direction returns both, as the library's route does.  Shared by
tests/test_conv_contract_gpu.py (runs every route on the GPU) and tests/test_conv_route.py (compares the C-ABI queries over a grid
of descriptors, no GPU needed).

The window kernels' minimum tile counts are read from the environment as the library reads them (tests/conftest.py sets both
to 1); every other threshold is restated at its default: a process that sets one of the other routing knobs routes differently."""
import os
from collections import namedtuple

from helpers import cdiv

WIN_MIN_TILES = int(os.environ.get('TOK_CONV_WIN_MIN_TILES', 128))
S2D_MIN_TILES = int(os.environ.get('TOK_CONV_S2D_MIN_TILES', 128))
PW_MIN_ROWS, SHORT_K = 100000, 400        # pw_min_rows(), short_k()
G256_MIN_TILES, G256_MIN_K = 128, 384     # gemm256_geometry, default rule

Geo = namedtuple('Geo', 'B H W C K R S P Q stride pad M Ktot x_bytes')     # ConvArgs as the launchers fill it


def geo_fwd(d):
    return Geo(d.n, d.h, d.w, d.c, d.k, d.r, d.s_pad, d.p, d.q, d.stride, d.pad, d.n * d.p * d.q, d.r * d.s_pad * d.c,
               d.n * d.h * d.w * d.c * 2)


def geo_dgrad(d):
    """dgrad_fill: the gathered tensor is dY (p x q x k), the output dX (h x w x c), stride 1, padding r - 1 - pad"""
    return Geo(d.n, d.p, d.q, d.k, d.c, d.r, d.s, d.h, d.w, 1, d.r - 1 - d.pad, d.n * d.h * d.w, d.r * d.s * d.k,
               d.n * d.p * d.q * d.k * 2)


def pick_bn(n_out, ktot, token_rows=False):
    if n_out <= 64:
        return 64
    if token_rows:
        return 128
    return 64 if ktot <= SHORT_K else 128


def pw_serves(bn, rows, c_red, n_out):
    return bn == 64 and rows >= PW_MIN_ROWS and c_red % 8 == 0 and n_out % 64 == 0


def _grid(cap, grid_m, grid_n):
    """plan_grid / pw_ring_grid / conv_win_grid / conv_s2d_grid: `cap` workgroups, never more than the tiles need, in units of
    8 * gridN"""
    unit, need = 8 * grid_n, grid_m * grid_n
    g = cap if need >= cap else cdiv(need, unit) * unit
    return max(g // unit * unit, unit)


def plan_grid(bn, gm, gn, per_cu=0):
    return _grid(256 * (per_cu or (3 if bn == 64 else 2)), gm, gn)


def ring_grid(bn, gm, gn):
    return _grid(256 * (2 if bn == 64 else 1), gm, gn)


def pick_tw(w):
    return 16 if w <= 16 else (32 if w <= 32 else 64)


def pick_wbn(k, ptiles):
    if k == 48:
        return 48
    if k <= 64:
        return 64
    if k % 96 == 0 and k % 128 != 0:
        return 96
    if k % 96 == 0 and ptiles * (k // 128) <= 256 and ptiles * (k // 96) <= 512:
        return 96
    return 128


def win_tiles(g):
    tw = pick_tw(g.W)
    gm = cdiv((g.M // (g.H * g.W)) * g.H, 256 // tw) * cdiv(g.W, tw)
    bn = pick_wbn(g.K, gm)
    return gm, cdiv(g.K, bn), tw, bn


def _win_common(g):
    if g.C % 8 or g.K % 8 or g.K < 32 or g.C < 32 or 64 < g.K < 96 or g.W < 12 or g.x_bytes >= 0x7FFFFFF0:
        return False
    return True


def win_serves(g, fused=False):
    if not (g.R == 3 and g.S == 3 and g.stride == 1 and g.pad == 1 and g.H == g.P and g.W == g.Q) or fused:
        return False
    gm, gn, _, _ = win_tiles(g)
    return _win_common(g) and gm * gn >= WIN_MIN_TILES


def s2d_tiles(g):
    tw = pick_tw(g.W)
    gm = 4 * cdiv((g.M // (g.P * g.Q)) * g.H, 256 // tw) * cdiv(g.W, tw)
    bn = pick_wbn(g.K, gm)
    return gm, cdiv(g.K, bn), tw, bn


def s2d_serves(g, stride, pad, fused=False):
    if not (g.R == 3 and g.S == 3 and stride == 2 and pad == 1) or fused:
        return False
    if g.P % 2 or g.Q % 2 or g.P != 2 * g.H or g.Q != 2 * g.W:
        return False
    gm, gn, _, _ = s2d_tiles(g)
    return _win_common(g) and gm * gn >= S2D_MIN_TILES


def g256_geometry(g):
    if not (g.R == 1 and g.S == 1 and g.stride == 1 and g.pad == 0 and g.C != 4):
        return False
    if g.Ktot % 8 or g.K % 8 or g.Ktot <= 64 or g.K < 192 or g.M < 4096:
        return False
    nt = cdiv(g.K, 256)
    if nt * 256 * 3 > g.K * 4 or cdiv(g.M, 256) * nt < G256_MIN_TILES:
        return False
    return g.Ktot >= G256_MIN_K


def g256_rows(g):
    return cdiv(cdiv(g.M, 256), 8) * 8


def stem_win_serves(g, bias, fused):
    if not (g.C == 4 and g.R == 7 and g.S == 8 and g.stride == 2 and g.pad == 3) or g.K % 8 or g.K > 64 or g.W % 2:
        return False
    return not bias and not fused and g.B * cdiv(g.P, 16) * cdiv(g.Q, 16) >= 16


def _pointwise(g):
    return g.R == 1 and g.S == 1 and g.stride == 1 and g.pad == 0 and g.C != 4


# (kernel name, statistics rows, pixels one tile holds, pixel tiles)
Route = namedtuple('Route', 'name rows tile_px tiles')


def _route_window(kern, tiles_of, g):
    gm, gn, tw, wbn = tiles_of(g)
    return Route(f'{kern}<{tw},{wbn}>', _grid(512, gm, gn) // gn, 256, gm)


def _route_gemm(g, pointwise, bn, gm, gather, act=False, bnep=False, sub=False):
    """route_gemm: the geometry's owner sizes the rows, the mode picks the kernel (`gather`: the name of the general mode)"""
    gn = cdiv(g.K, bn)
    ring_owns = pointwise and pw_serves(bn, g.M, g.C, g.K)
    g256_owns = pointwise and not ring_owns and g256_geometry(g)
    if g256_owns:
        sized = (g256_rows(g), 256, g256_rows(g))
        if not (act or bnep or sub):
            return Route('gemm256', *sized)
    else:
        sized = ((ring_grid if ring_owns else plan_grid)(bn, gm, gn) // gn, 128, gm)
    bt = 64 if bnep else bn
    if pointwise and pw_serves(bt, g.M, g.C, g.K):
        return Route('igemm<128,64,pw3>@ring_grid' if act else ('ring<64,bnep>' if bnep else 'ring<64>'), *sized)
    if sub or ((act or bnep) and not pointwise):
        return Route('refused', *sized)
    if pointwise:
        return Route(f'igemm<128,{bt},pw{3 if act else 4 if bnep else 1}>' + ('@g256_layer' if g256_owns else ''), *sized)
    return Route(f'igemm<128,{bt},{gather}>', *sized)


def route_fwd(d, bias=False, act=False, bnep=False):
    """route_fwd: the kernel a forward entry runs and the rows tok_conv_fwd_stat_rows announces"""
    g, c4 = geo_fwd(d), d.c == 4
    if not c4 and not bnep and win_serves(g, act):
        return _route_window('conv_win', win_tiles, g)
    bn = pick_bn(d.k, g.Ktot, d.h == 1 and d.w == 1)
    r = _route_gemm(g, _pointwise(g), bn, cdiv(g.M, 128), 'c4' if c4 else 'gather', act, bnep)
    if c4 and not bnep and stem_win_serves(g, bias, act):
        return r._replace(name='stem_win')
    return r


def dgrad_plan(d):
    g = geo_dgrad(d)
    bn = pick_bn(d.c, g.Ktot, d.h == 1 and d.w == 1)
    if d.stride == 1:
        gm = cdiv(g.M, 128)
    else:
        gm = 4 * max(cdiv(d.n * ((d.h - ph + 1) // 2) * ((d.w - pw + 1) // 2), 128) for ph in (0, 1) for pw in (0, 1))
    return g, bn, gm, cdiv(d.c, bn)


def route_dgrad(d, act=False, sub=False):
    """route_dgrad: the kernel a data-gradient entry runs and the rows tok_conv_dgrad_stat_rows announces"""
    g, bn, gm, _ = dgrad_plan(d)
    if d.stride == 1 and win_serves(g, act or sub):
        return _route_window('conv_win', win_tiles, g)
    if d.stride == 2 and s2d_serves(g, d.stride, d.pad, act or sub):
        return _route_window('conv_s2d', s2d_tiles, g)
    return _route_gemm(g, d.stride == 1 and _pointwise(g), bn, gm, f'gather_s{d.stride}', act=act, sub=sub)


def dgrad2_ok(d1, d2):
    """tok_conv_dgrad2_ok: two pointwise layers over the same pixels whose second sits on the 64-wide ring (tile picked as for a map)"""
    for d in (d1, d2):
        if not (d.r == 1 and d.s == 1 and d.stride == 1 and d.pad == 0 and d.k % 8 == 0 and d.c % 64 == 0):
            return False
    if (d1.n, d1.h, d1.w, d1.c) != (d2.n, d2.h, d2.w, d2.c):
        return False
    rows = d1.n * d1.h * d1.w
    return pick_bn(d2.c, d2.k) == 64 and pw_serves(64, rows, d1.k, d1.c) and pw_serves(64, rows, d2.k, d2.c)


ROUTES_FWD = ({f'igemm<128,{bn},{m}>' for bn in (64, 128) for m in ('gather', 'pw1', 'pw3')} |
              {'igemm<128,64,pw4>', 'igemm<128,64,c4>', 'stem_win', 'ring<64>', 'ring<64,bnep>', 'igemm<128,64,pw3>@ring_grid',
               'gemm256', 'igemm<128,64,pw4>@g256_layer', 'igemm<128,128,pw3>@g256_layer'} |
              {f'conv_win<{tw},{bn}>' for tw in (16, 32, 64) for bn in (48, 64, 96, 128)})
ROUTES_DGRAD = ({f'igemm<128,{bn},{m}>' for bn in (64, 128) for m in ('gather_s1', 'gather_s2', 'pw1')} | {'ring<64>', 'gemm256'} |
                {f'{kern}<{tw},{bn}>' for kern in ('conv_win', 'conv_s2d') for tw in (16, 32, 64) for bn in (48, 64, 96, 128)})
ACT_ROUTES = {'pw1_64': 'igemm<128,64,pw3>', 'pw1_128': 'igemm<128,128,pw3>', 'ring_256to64': 'igemm<128,64,pw3>@ring_grid',
              'g256': 'igemm<128,128,pw3>@g256_layer'}
