"""The weight-gradient planner (make_plan, csrc/conv_wgrad.hip) without a GPU: tok_conv_wgrad_ws_bytes, tok_conv_wgrad_bias_ws_bytes
and tok_conv_wgrad_bias_ok are pure host arithmetic, so the library answers them on any machine.  They are compared with the
restated plan (tests/conv_wgrad_plan_ref.py) on the cases of the GPU contract test and over a fixed grid of descriptors that
crosses every threshold of make_plan from both sides.

The restatement is of the defaults and the library reads its knobs once per process: the module refuses to run in a process
that sets one of them."""
import ctypes
import itertools
import os

from conv_wgrad_plan_ref import ROUTES_WGRAD, WGRAD_CASES, make_plan
from helpers import conv_desc
from torchok_amd import _C

KNOBS = ('TOK_WGRAD_TAPS_WGS', 'TOK_WGRAD_WGS', 'TOK_WGRAD_WGS_LONG', 'TOK_WGRAD_256', 'TOK_WGRAD_2BUF_WGS')

BATCHES = (1, 2, 24, 256)
MAPS = ((1, 1), (2, 2), (5, 3), (7, 7), (14, 14), (16, 16), (9, 33), (33, 35), (56, 56), (64, 96), (70, 72), (128, 256))
WIDTHS = (8, 40, 48, 64, 96, 128, 136, 192, 256, 384, 720, 1024, 2048)
FILTERS = ((1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1), (2, 2, 0), (7, 2, 3))       # (r, stride, pad)


def _grid():
    """(n, h, w, c, k, r, stride, pad)"""
    for n, (h, w), c, k, f in itertools.product(BATCHES, MAPS, WIDTHS, WIDTHS, FILTERS):
        yield (n, h, w, c, k) + f
    for n, (h, w), k in itertools.product(BATCHES, MAPS, WIDTHS):                    # the 4-channel image: the stem filter only
        yield (n, h, w, 4, k, 7, 2, 3)


def _boundaries():
    # rows M on both sides of 100 000 (64 rows per barrier of the two-buffer kernel) and 200 000 (the 256 x 256 ring tile; its
    # ragged-tile rule: 264 / 384 wide fail it, 512 / 720 pass)
    for m in (99999, 100000, 199999, 200000):
        for c, k in itertools.product((248, 256, 264, 384, 512, 720), repeat=2):
            yield (1, 1, m, c, k, 1, 1, 0)
        for c, k in ((40, 136), (128, 128), (136, 120), (64, 64), (48, 48)):
            yield (1, 1, m, c, k, 3, 1, 1)
            yield (1, 3, m, c, k, 3, 1, 1)
    # 2^30 bytes of x or dy: the window kernel stops there (64-wide layers fall to the per-tap kernel, 48-wide ones to two buffers)
    for w in (2047, 2048):
        yield (2, 2048, w, 64, 64, 3, 1, 1)          # x and dy cross together
        yield (2, 2048, w, 128, 64, 3, 1, 1)         # x alone over
        yield (1, 2048, w, 64, 128, 3, 1, 1)         # dy alone at the bound
        yield (2, 1024, w, 64, 128, 3, 1, 1)
    for w in (11184810, 11184811):                   # 2^30 / 96 = 11 184 810.67
        yield (1, 1, w, 48, 48, 3, 1, 1)
        yield (1, 1, w // 2 + 1, 96, 48, 3, 1, 1)
        yield (1, 1, w // 2 + 1, 48, 96, 3, 1, 1)
    # ring tiles: k = 64 / 72, Ktot = 64 / 72 / 128 / 256 and their neighbours
    for c, k in itertools.product((56, 64, 72, 120, 128, 136, 248, 256, 264), (56, 64, 72, 120, 128, 136, 248, 256, 264)):
        yield (2, 16, 16, c, k, 1, 1, 0)
        yield (2, 16, 16, c, k, 1, 2, 0)             # two-buffer tiles: k, Ktot = 128
        yield (2, 16, 16, c, k, 3, 2, 1)
    # the stem window kernel: k <= 64, even width, 16 pixel tiles of 8 x 16 at least
    for n, (h, w), k in itertools.product((1, 2), ((64, 128), (64, 96), (64, 127), (50, 128), (48, 128), (2, 2)), (8, 56, 64, 72)):
        yield (n, h, w, 4, k, 7, 2, 3)
    # splits: 8 stages per workgroup against the caps (256 / 512 splits) and the targets
    for m in (1, 31, 32, 33, 255, 256, 257, 8 * 32 * 256 - 1, 8 * 32 * 256, 8 * 32 * 256 + 1, 8 * 32 * 512, 8 * 32 * 512 + 1,
              8 * 64 * 256, 8 * 64 * 256 + 1):
        for c, k, f in ((64, 64, (1, 1, 0)), (64, 64, (3, 1, 1)), (8, 8, (3, 1, 1)), (40, 136, (3, 1, 1)), (2048, 2048, (1, 1, 0))):
            yield (1, 1, m, c, k) + f
        yield (1, 1, 2 * m, 4, 64, 7, 2, 3)


def _served(geo):
    """what tok_conv_wgrad itself accepts: padded channel counts (the helper stores the taps of c == 4 eight wide, as the entry
    point asks); a filter that does not fit the padded map has no output pixel and is no convolution"""
    n, h, w, c, k, r, stride, pad = geo
    return k % 8 == 0 and (c % 8 == 0 or c == 4) and h + 2 * pad >= r and w + 2 * pad >= r


def _check(lib, geo):
    d = conv_desc(*geo)
    p = make_plan(d)
    ws_bytes = p.splitM * d.k * d.r * d.s_pad * d.c * 4
    D = ctypes.byref(d)
    got = (lib.tok_conv_wgrad_ws_bytes(D), lib.tok_conv_wgrad_bias_ok(D), lib.tok_conv_wgrad_bias_ws_bytes(D))
    assert got == (ws_bytes, int(p.ring), ws_bytes + p.splitM * d.k * 4), (geo, p, got)
    return p.kernel


def test_defaults_only():
    assert not [v for v in KNOBS if v in os.environ], 'unset the TOK_WGRAD_* knobs: the plan is restated at its defaults'


def test_queries_equal_the_restated_plan_on_the_contract_cases():
    lib = _C.load_library()
    for name, geo, _, _, kernel in WGRAD_CASES:
        assert _check(lib, geo) == kernel, name


def test_queries_equal_the_restated_plan_over_the_grid():
    lib = _C.load_library()
    seen, count = set(), 0
    for geo in itertools.chain(_grid(), _boundaries()):
        if not _served(geo):
            continue
        seen.add(_check(lib, geo))
        count += 1
    assert count >= 2000, count
    assert ROUTES_WGRAD <= seen, ROUTES_WGRAD - seen
