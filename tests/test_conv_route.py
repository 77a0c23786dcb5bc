"""The route of the convolution forward and data gradient (route_fwd / route_dgrad, csrc/conv_igemm.hip) without a GPU:
tok_conv_fwd_stat_rows, tok_conv_dgrad_stat_rows, tok_conv_dgrad_subacc_ok and tok_conv_dgrad2_ok are pure host arithmetic, so the
library answers them on any machine.  They are compared with the restated route (tests/conv_route_ref.py) on the cases of the GPU
contract test and over a fixed grid of descriptors that crosses every threshold of the route from both sides.  The statistics
rows depend on the geometry alone; the kernel's name also on the mode, so every descriptor is named under every mode.

The restatement reads the window kernels' minimum tile counts as the library does (tests/conftest.py sets both to 1) and is of
the defaults otherwise; the library reads its knobs once per process: the module refuses to run in a process that sets one of
the others."""
import ctypes
import itertools
import os

from conv_route_ref import ACT_ROUTES, ROUTES_DGRAD, ROUTES_FWD, dgrad2_ok, route_dgrad, route_fwd
from helpers import ERR_INVALID, conv_desc
from test_conv_contract_gpu import DGRAD_CASES, FWD_CASES
from torchok_amd import _C

KNOBS = ('TOK_SHORT_K', 'TOK_PW_RING_MIN_ROWS', 'TOK_GEMM256', 'TOK_GEMM256_MIN_K', 'TOK_GEMM256_MIN_TILES')

BATCHES = (1, 2, 24, 256)
MAPS = ((1, 1), (2, 2), (5, 3), (7, 7), (14, 14), (16, 16), (9, 33), (33, 35), (56, 56), (64, 96), (70, 72), (128, 256))
WIDTHS = (8, 40, 48, 64, 96, 128, 136, 192, 256, 384, 720, 1024, 2048)
FILTERS = ((1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1), (2, 2, 0), (7, 2, 3))       # (r, stride, pad)
FWD_MODES = (dict(), dict(bias=True), dict(act=True), dict(bnep=True))
DGRAD_MODES = (dict(), dict(act=True), dict(sub=True))


def _grid():
    """(n, h, w, c, k, r, stride, pad)"""
    for n, (h, w), c, k, f in itertools.product(BATCHES, MAPS, WIDTHS, WIDTHS, FILTERS):
        yield (n, h, w, c, k) + f
    for n, (h, w), k in itertools.product(BATCHES, MAPS, WIDTHS):                    # the 4-channel image: the stem filter only
        yield (n, h, w, 4, k, 7, 2, 3)


def _boundaries():
    # the pointwise ring: TOK_PW_RING_MIN_ROWS 100 000 rows, 64-wide tiles only (outputs up to 64 wide, or a reduction up to
    # short_k = 400), outputs a multiple of 64; behind it the 256 x 256 tiles
    for m in (99999, 100000):
        for c, k in itertools.product((64, 72, 128, 392, 400, 408, 512), (56, 64, 72, 128, 192, 256)):
            yield (1, 1, m, c, k, 1, 1, 0)
            yield (1, 1, m, k, c, 1, 1, 0)
    # gemm256_geometry: 4096 rows, 192 outputs, a reduction of 384, 128 tiles, a last channel tile at least a quarter full
    for m in (4095, 4096, 8191, 8192, 8193, 16383, 16384, 16385, 32768):
        for c, k in itertools.product((376, 384, 392, 408, 1024), (184, 192, 256, 320, 328, 336, 384, 512, 1024)):
            yield (1, 1, m, c, k, 1, 1, 0)
            yield (1, 1, m, k, c, 1, 1, 0)
    # the window kernels: 3x3 maps 11 / 12 / 16 / 17 / 32 / 33 wide, 24 ... 136 channels, tile counts about the default minimum 128
    for w, c, k in itertools.product((11, 12, 16, 17, 32, 33, 64, 65), (24, 32, 64), (24, 32, 48, 64, 72, 88, 96, 128, 136, 192, 384)):
        for n, h in ((1, 16), (2, 64), (8, 127), (8, 128), (8, 129)):
            yield (n, h, w, c, k, 3, 1, 1)
            yield (n, h, w, k, c, 3, 1, 1)
            yield (n, 2 * h, 2 * w, c, k, 3, 2, 1)
            yield (n, 2 * h, 2 * w, k, c, 3, 2, 1)
            yield (n, 2 * h + 1, 2 * w, c, k, 3, 2, 1)                  # odd extents: off the stride-2 window kernel
    for w in (2047, 2048):                          # 2^31 bytes of the gathered tensor: the window offsets stop there
        yield (2, 2048, w, 128, 64, 3, 1, 1)
        yield (2, 2048, w, 64, 128, 3, 1, 1)
    # the stem window kernel: k <= 64, even width, 16 tiles of 16 x 16 at least; its grid against the rows
    for n, (h, w), k in itertools.product((1, 2, 64), ((64, 128), (64, 96), (64, 127), (50, 128), (48, 128), (2, 2), (224, 224)),
                                          (8, 56, 64, 72)):
        yield (n, h, w, 4, k, 7, 2, 3)


def _served(geo):
    """what check_desc accepts: padded channel counts; a filter that does not fit the padded map is no convolution"""
    n, h, w, c, k, r, stride, pad = geo
    return k % 8 == 0 and (c % 8 == 0 or c == 4) and h + 2 * pad >= r and w + 2 * pad >= r


def _dgrad_served(d):
    """... and dgrad_fill: no data gradient of the stem image, strides 1 and 2, padding inside the filter, dy and w below 4 GiB"""
    return (d.c % 8 == 0 and d.stride in (1, 2) and d.pad <= d.r - 1 and d.n * d.p * d.q * d.k * 2 < 0xFFFFFFF0
            and d.c * d.r * d.s * d.k * 2 < 0xFFFFFFF0)


def _modes(modes, d):
    """the fused modes exist on pointwise layers only: the entry points refuse them elsewhere, by name"""
    pointwise = d.r == 1 and d.stride == 1 and d.pad == 0 and d.c != 4
    return [m for m in modes if pointwise or not (m.get('act') or m.get('bnep') or m.get('sub'))]


def _check_fwd(lib, geo):
    d = conv_desc(*geo)
    routes = [route_fwd(d, **mode) for mode in _modes(FWD_MODES, d)]
    assert len({r.rows for r in routes}) == 1, (geo, routes)                # the geometry alone sizes the rows
    assert lib.tok_conv_fwd_stat_rows(ctypes.byref(d)) == routes[0].rows, (geo, routes[0])
    return {r.name for r in routes}


def _check_dgrad(lib, geo):
    d = conv_desc(*geo)
    D = ctypes.byref(d)
    if not _dgrad_served(d):
        assert lib.tok_conv_dgrad_stat_rows(D) == ERR_INVALID and lib.tok_conv_dgrad_subacc_ok(D) == 0, geo
        return None
    routes = [route_dgrad(d, **mode) for mode in _modes(DGRAD_MODES, d)]
    assert len({r.rows for r in routes}) == 1, (geo, routes)
    assert lib.tok_conv_dgrad_stat_rows(D) == routes[0].rows, (geo, routes[0])
    assert lib.tok_conv_dgrad_subacc_ok(D) == int(routes[-1].name == 'ring<64>'), (geo, routes[-1])
    return {r.name for r in routes}


def _check_dgrad2(lib, geo):
    """the pair of the fused residual unit: (c -> k) and (c -> c) over the same pixels, and the pair the other way round"""
    n, h, w, c, k, r, stride, pad = geo
    if (r, stride, pad) != (1, 1, 0):
        return 0
    d1, d2 = conv_desc(n, h, w, c, k, 1, 1, 0), conv_desc(n, h, w, c, c, 1, 1, 0)
    for a, b in ((d1, d2), (d2, d1)):
        assert lib.tok_conv_dgrad2_ok(ctypes.byref(a), ctypes.byref(b)) == int(dgrad2_ok(a, b)), geo
    return int(dgrad2_ok(d1, d2)) + 2 * int(dgrad2_ok(d2, d1))


def test_defaults_only():
    assert not [v for v in KNOBS if v in os.environ], 'unset the routing knobs: the route is restated at its defaults'


def test_queries_equal_the_restated_route_on_the_contract_cases():
    lib = _C.load_library()
    for name, geo, entry, route in FWD_CASES:
        assert route in _check_fwd(lib, geo), name
    for name, geo, route, _ in DGRAD_CASES:
        names = _check_dgrad(lib, geo)
        assert route in names and (name not in ACT_ROUTES or ACT_ROUTES[name] in names), name


def test_queries_equal_the_restated_route_over_the_grid():
    lib = _C.load_library()
    seen_f, seen_d, count_f, count_d, pairs = set(), set(), 0, 0, set()
    for geo in itertools.chain(_grid(), _boundaries()):
        if not _served(geo):
            continue
        seen_f |= _check_fwd(lib, geo)
        count_f += 1
        names = _check_dgrad(lib, geo)
        if names is not None:
            seen_d |= names
            count_d += 1
            pairs.add(_check_dgrad2(lib, geo))
    assert count_f >= 2000 and count_d >= 2000, (count_f, count_d)
    assert ROUTES_FWD <= seen_f, ROUTES_FWD - seen_f
    assert ROUTES_DGRAD <= seen_d, ROUTES_DGRAD - seen_d
    assert pairs == {0, 1, 2, 3}, pairs              # tok_conv_dgrad2_ok answered yes and no, in either order of the pair
