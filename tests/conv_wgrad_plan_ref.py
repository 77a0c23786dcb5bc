"""make_plan (csrc/conv_wgrad.hip) and stem_wgrad_serves (csrc/stem.hip) restated, every threshold at its default: which
kernel a layer's weight gradient takes, its tiles, how the reduction rows are split and hence the workspace the C-ABI queries
ask for.  Shared by tests/test_conv_wgrad_contract_gpu.py (runs every route on the GPU) and tests/test_conv_wgrad_plan.py
(compares the queries over a grid of descriptors, no GPU needed).  The restatement is of the defaults: a process that sets one
of the TOK_WGRAD_* split / tile knobs plans differently."""
from collections import namedtuple

from helpers import cdiv

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
