#!/usr/bin/env python
"""Bit-for-bit A/B of every entry of the resampling and loss kernels (resample.hip, fuse_sum.hip, neck_resample.hip, loss_*.hip,
the counts of metric.hip) between two builds of the library: run once per library with --save, the second time with --cmp.
    tools/ab_lib.sh <parent>
    TOK_LIB=torchok_amd/lib/libtok_ab.so python tools/ubench/resample_loss_check.py --save /tmp/rl_a.pt
    python tools/ubench/resample_loss_check.py --save /tmp/rl_b.pt --cmp /tmp/rl_a.pt
Inputs are real-valued (randn from a seeded CPU generator: both runs see the same bits, and a changed fp contraction shows only
on non-dyadic data); every output buffer, pads and fp64 part slots included, is kept and compared as raw integers.
--time prints microseconds per call (device events, after warm-up, over at least 0.5 s of work) of the three gather backward
kernels at one user-sized shape each, instead of the bit check."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from torchok_amd import _C  # noqa: E402

LOSS_FLOATS = 2050      # TOK_CE_LOSS_FLOATS
CE_PARTS = 512
IGNORE = 255
# the geometries of tests/test_resample_contract_gpu.py, test_nearest_contract_gpu.py, test_loss_contract_gpu.py and
# test_resample_tiled_contract_gpu.py
BIL_SIZES = [((1, 1), (2, 2)), ((8, 8), (16, 16)), ((2, 4), (16, 32)), ((5, 7), (13, 20)), ((7, 5), (7, 10)), ((9, 9), (4, 5)),
             ((3, 3), (1, 1)), ((8, 8), (8, 8))]
BIL_CHANNELS = [(8, 0, 8, 8), (8, 24, 16, 40), (64, 24, 72, 96), (3, 5, 5, 11), (18, 18, 24, 56), (8, 4, 8, 16)]
NEAR_SIZES = [((1, 1), (2, 2)), ((3, 2), (6, 4)), ((5, 4), (6, 4)), ((7, 5), (13, 9)), ((9, 7), (9, 7)), ((6, 4), (3, 2))]
NEAR_CHANNELS = [(8, 0, 8, 8), (8, 24, 16, 40), (64, 0, 64, 64), (64, 24, 72, 96), (3, 5, 5, 11), (18, 5, 19, 27)]
UP_WIDTHS = [(3, 8), (8, 8), (13, 16), (19, 24), (25, 32), (32, 32)]
UP_GEOM = [(2, 8, 8, 32, 32), (2, 8, 8, 33, 33), (2, 4, 6, 32, 48), (2, 8, 4, 16, 32), (2, 9, 13, 36, 52), (2, 3, 5, 12, 20),
           (2, 1, 7, 4, 28), (2, 16, 16, 16, 16), (2, 16, 24, 8, 12), (2, 16, 16, 5, 5), (3, 17, 17, 68, 68)]


def _by_factor(h, w, fs):
    return [(h // f, w // f) for f in fs]


# (n, h, w, c, sources): tiled geometries first, then the ones the generic kernels serve
NECK = ([(2, 32, 32, 40, _by_factor(32, 32, (2, 4, 8))), (2, 24, 40, 24, [(12, 20), (6, 10), (3, 5)]),
         (1, 16, 16, 8, _by_factor(16, 16, (2, 4, 8))), (2, 48, 48, 40, _by_factor(48, 48, (8, 2, 4))),
         (1, 16, 32, 32, _by_factor(16, 32, (2, 4, 8)))] +
        [(1, 32, 16, 72, _by_factor(32, 16, f)) for f in ((2,), (4,), (8,), (2, 4), (2, 8), (4, 8))] +
        [(1, 32, 32, 16, [(16, 16), (16, 16)]), (1, 32, 32, 16, [(11, 11)]), (1, 32, 32, 16, [(16, 8)]), (1, 32, 32, 8, [(2, 2)]),
         (1, 24, 24, 8, [(12, 12), (6, 6), (3, 3)]), (2, 13, 20, 24, [(5, 7)]), (1, 8, 8, 2056, [(4, 4)]), (1, 16, 16, 12, [(8, 8)])])

GEN = torch.Generator().manual_seed(20240607)


def randn(*shape, dtype=torch.bfloat16):
    return torch.randn(*shape, generator=GEN).to(dtype).cuda()


def labels(shape, classes, ignored=0.1):
    t = torch.randint(0, classes, shape, generator=GEN)
    t[torch.rand(shape, generator=GEN) < ignored] = IGNORE
    return t.cuda()


def P(t):
    return None if t is None else t.data_ptr()


class Run:
    def __init__(self):
        self.lib = _C.load_library()
        self.st = torch.cuda.current_stream().cuda_stream
        self.out = {}

    def call(self, name, *args):
        rc = getattr(self.lib, name)(*args, self.st)
        assert rc == 0, (name, self.lib.tok_last_error())

    def keep(self, key, *tensors):
        torch.cuda.synchronize()
        for i, t in enumerate(tensors):
            raw = t.detach().contiguous().view(-1).view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
            self.out[f'{key}/{i}'] = raw.cpu()


def gather_pairs(r):
    for kind, sizes, channels in (('bilinear', BIL_SIZES, BIL_CHANNELS), ('nearest', NEAR_SIZES, NEAR_CHANNELS)):
        for (hs, ws), (hd, wd) in sizes:
            for c, off, ld_src, ld_dst in channels:
                n, key = 3, f'{kind}/{hs}x{ws}-{hd}x{wd}/c{c}o{off}'
                src, dst = randn(n, hs, ws, ld_src), randn(n, hd, wd, ld_dst)
                r.call(f'tok_{kind}_fwd', P(src), n, hs, ws, c, ld_src, P(dst), hd, wd, ld_dst, off)
                r.keep(key + '/fwd', dst)
                for acc in (0, 1):
                    dsrc = randn(n, hs, ws, ld_src)
                    r.call(f'tok_{kind}_bwd', P(dst), n, hd, wd, ld_dst, off, P(dsrc), hs, ws, c, ld_src, acc)
                    r.keep(f'{key}/bwd{acc}', dsrc)


def fuse_pair(r):
    n, h, w, c, shifts = 2, 16, 16, 24, (0, 1, 2)
    terms = [randn(n, h >> s, w >> s, c) for s in shifts]
    scale = [torch.randn(c, generator=GEN).cuda() for _ in shifts]
    shift = [torch.randn(c, generator=GEN).cuda() for _ in shifts]
    for affine in (0, 1):
        for relu in (0, 1):
            out, mask = randn(n, h, w, c), torch.zeros(n * h * w * c // 8, dtype=torch.uint8).cuda()
            args = []
            for j, s in enumerate(shifts):
                args += [P(terms[j]), s, P(scale[j]) if affine else None, P(shift[j]) if affine else None]
            r.call('tok_fuse_sum_affine_relu_fwd', *args, None, 0, None, None, n, h, w, c, relu, P(out), P(mask))
            r.keep(f'fuse/fwd/a{affine}r{relu}', out, mask)
            for s in shifts:
                for acc in (0, 1):
                    for m in (mask, None):
                        dterm = randn(n, h >> s, w >> s, c)
                        r.call('tok_fuse_sum_relu_bwd', P(out), P(m), n, h, w, c, s, P(dterm), acc)
                        r.keep(f'fuse/bwd/a{affine}r{relu}s{s}acc{acc}m{int(m is not None)}', dterm)


def neck(r):
    for n, h, w, c, lows in NECK:
        key = f'neck/{n}x{h}x{w}x{c}/' + '_'.join(f'{a}x{b}' for a, b in lows)
        y0, y = randn(n, h, w, c), randn(n, h, w, c)
        ts = [randn(n, a, b, c) for a, b in lows]
        srcs = [v for t, (a, b) in zip(ts, lows) for v in (P(t), a, b)] + [None, 0, 0] * (3 - len(lows))
        if c % 8 == 0:
            rows = r.lib.tok_bilinear_sum_stats_rows(n, h, w, c)
            stats = torch.zeros(2, rows, c).cuda()
            r.call('tok_bilinear_sum_stats', P(y0), *srcs, n, h, w, c, P(y), P(stats))
            r.keep(key + '/sum', y, stats)
            r.call('tok_bilinear_sum_stats', P(y), *srcs, n, h, w, c, P(y), None)      # in place, no statistics
            r.keep(key + '/sum_inplace', y)
        ds = [randn(n, a, b, c) for a, b in lows]
        dsts = [v for t, (a, b) in zip(ds, lows) for v in (P(t), a, b)] + [None, 0, 0] * (3 - len(lows))
        r.call('tok_bilinear_bwd_multi', P(y0), n, h, w, c, *dsts)
        r.keep(key + '/adj', *ds)


def upsample_ce(r):
    gscale = torch.tensor([1.3]).cuda()
    for n, hs, ws, hd, wd in UP_GEOM:
        for classes, ld in UP_WIDTHS:
            key = f'upce/{n}x{hs}x{ws}-{hd}x{wd}/c{classes}'
            low, tgt = randn(n, hs, ws, ld), labels((n, hd, wd), classes)
            lse, row_loss, loss = torch.zeros(n * hd * wd).cuda(), torch.zeros(n * hd * wd).cuda(), torch.zeros(LOSS_FLOATS).cuda()
            r.call('tok_upsample_ce_fwd', P(low), n, hs, ws, classes, ld, hd, wd, P(tgt), IGNORE, P(lse), P(row_loss), P(loss))
            r.keep(key + '/fwd', lse, row_loss, loss)
            for acc in (0, 1):
                dlow = randn(n, hs, ws, ld)
                r.call('tok_upsample_ce_bwd', P(low), n, hs, ws, classes, ld, hd, wd, P(tgt), IGNORE, P(lse), P(loss), P(gscale),
                       P(dlow), acc)
                r.keep(f'{key}/bwd{acc}', dlow)


def softmax_ce(r):
    gscale = torch.tensor([0.7]).cuda()
    for rows, classes, ld, smooths in ((5000, 100, 104, (0.0, 0.1)), (16421, 19, 24, (0.0, 0.1)), (4096 * CE_PARTS + 4097, 3, 8, (0.0,))):
        z, tgt = randn(rows, ld), labels((rows,), classes)
        for smooth in smooths:
            lse, row_loss, loss = torch.zeros(rows).cuda(), torch.zeros(rows).cuda(), torch.zeros(LOSS_FLOATS).cuda()
            r.call('tok_softmax_ce_smooth_fwd', P(z), P(tgt), rows, classes, ld, IGNORE, smooth, P(lse), P(row_loss), P(loss))
            dz = randn(rows, ld)
            r.call('tok_softmax_ce_smooth_bwd', P(z), P(tgt), P(lse), P(loss), P(gscale), rows, classes, ld, IGNORE, smooth, P(dz))
            r.keep(f'ce/{rows}x{classes}/s{smooth}', lse, row_loss, loss, dz)


def pointwise(r):
    gscale = torch.tensor([0.7]).cuda()
    rows, classes, ld = 1100, 9, 16
    z = randn(rows, ld)
    tgt = (torch.rand(rows, classes, generator=GEN) < 0.5).float()
    tgt[torch.rand(rows, classes, generator=GEN) < 0.1] = -1.0
    for name, t in (('some', tgt.cuda()), ('all_ignored', torch.full((rows, classes), -1.0).cuda())):
        for mean in (1, 0):
            loss, dz = torch.zeros(LOSS_FLOATS).cuda(), randn(rows, ld)
            r.call('tok_bce_logits_fwd', P(z), P(t), rows, classes, ld, -1.0, mean, P(loss))
            r.call('tok_bce_logits_bwd', P(z), P(t), P(loss), P(gscale), rows, classes, ld, -1.0, mean, P(dz))
            r.keep(f'bce/{name}/mean{mean}', loss, dz)
    n = 20001
    x, t = randn(n), torch.randn(n, generator=GEN).cuda()
    for kind in range(4):
        for mean in (1, 0):
            loss, dx = torch.zeros(LOSS_FLOATS).cuda(), randn(n)
            r.call('tok_regression_loss_fwd', P(x), P(t), n, kind, 0.75, mean, P(loss))
            r.call('tok_regression_loss_bwd', P(x), P(t), P(gscale), n, kind, 0.75, mean, P(dx))
            r.keep(f'reg/k{kind}/mean{mean}', loss, dx)


def dice_and_counts(r):
    gscale = torch.tensor([0.7]).cuda()
    rows = 5000
    for mode, classes, ld in ((0, 19, 24), (1, 1, 8), (2, 7, 8)):
        z = randn(rows, ld)
        if mode == 0:
            tgt = torch.randint(0, classes, (rows,), generator=GEN).cuda()
        else:
            tgt = (torch.rand(rows, classes, generator=GEN) < 0.4).float().cuda()
        g = r.lib.tok_dice_rows(rows)
        partial, loss, coef, dz = torch.zeros(g * 3 * classes).cuda(), torch.zeros(2).cuda(), torch.zeros(2 * classes).cuda(), randn(rows, ld)
        r.call('tok_dice_fwd', P(z), P(tgt), rows, classes, ld, mode, 0.5, 1e-7, mode == 2, None, 0, P(partial), P(loss), P(coef))
        r.call('tok_dice_bwd', P(z), P(tgt), P(coef), P(gscale), rows, classes, ld, mode, P(dz))
        r.keep(f'dice/m{mode}', partial, loss, coef, dz)
    classes, ld = 19, 24
    z, tgt = randn(rows, ld), labels((rows,), classes)
    counts, confusion = torch.zeros(3 * classes, dtype=torch.int64).cuda(), torch.zeros(classes * classes, dtype=torch.int64).cuda()
    r.call('tok_cls_stats_update', P(z), None, P(tgt), rows, classes, ld, IGNORE, P(counts))
    r.call('tok_confusion_update', P(z), None, P(tgt), rows, classes, ld, IGNORE, P(confusion))
    r.keep('counts', counts, confusion)


def time_call(fn):
    """microseconds per call: 10 warm-up calls, then batches between two events until 0.5 s of device time"""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    total_ms, calls, batch = 0.0, 0, 10
    while total_ms < 500.0:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        total_ms += a.elapsed_time(b)
        calls += batch
        batch = min(batch * 2, 1000)
    return 1e3 * total_ms / calls


def timing(r):
    """one user-sized shape per kernel whose code moved (HRNet segmentation at 512 x 1024, batch 8)"""
    g = torch.Generator(device='cuda').manual_seed(1)
    rn = lambda *s: torch.randn(*s, device='cuda', generator=g).to(torch.bfloat16)      # noqa: E731
    gscale = torch.tensor([1.0]).cuda()
    res = []
    n, hs, ws, hd, wd = 8, 128, 256, 512, 1024
    for name, c in (('bilinear_bwd_16B_c24', 24), ('bilinear_bwd_scalar_c270', 270)):
        ddst, dsrc = rn(n, hd, wd, c), rn(n, hs, ws, c)
        res.append((name, time_call(lambda: r.call('tok_bilinear_bwd', P(ddst), n, hd, wd, c, 0, P(dsrc), hs, ws, c, c, 0))))
        del ddst, dsrc
    hs, ws, classes, ld = 103, 205, 19, 24      # a ratio the tiled form does not serve: the gather kernel
    low, dlow = rn(n, hs, ws, ld), rn(n, hs, ws, ld)
    tgt = torch.randint(0, classes, (n, hd, wd), device='cuda', generator=g)
    lse, row_loss, loss = torch.zeros(n * hd * wd).cuda(), torch.zeros(n * hd * wd).cuda(), torch.zeros(LOSS_FLOATS).cuda()
    r.call('tok_upsample_ce_fwd', P(low), n, hs, ws, classes, ld, hd, wd, P(tgt), IGNORE, P(lse), P(row_loss), P(loss))
    res.append(('upsample_ce_bwd_gather', time_call(lambda: r.call(
        'tok_upsample_ce_bwd', P(low), n, hs, ws, classes, ld, hd, wd, P(tgt), IGNORE, P(lse), P(loss), P(gscale), P(dlow), 0))))
    for name, us in res:
        print(f'{name} {us:.2f} us', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--save', default=None)
    ap.add_argument('--cmp', default=None)
    ap.add_argument('--time', action='store_true')
    args = ap.parse_args()
    r = Run()
    print('library:', _C.LIB_PATH, flush=True)
    if args.time:
        timing(r)
        return
    assert args.save, '--save FILE (or --time)'
    for family in (gather_pairs, fuse_pair, neck, upsample_ce, softmax_ce, pointwise, dice_and_counts):
        family(r)
        print(f'{family.__name__}: {len(r.out)} buffers so far', flush=True)
    torch.save(r.out, args.save)
    if args.cmp:
        other = torch.load(args.cmp)
        assert other.keys() == r.out.keys(), 'the two runs kept different buffers'
        bad = [k for k in r.out if not torch.equal(r.out[k], other[k])]
        print(f'{len(r.out)} buffers, bit-identical to {args.cmp}:', 'ALL' if not bad else f'NO, {len(bad)} differ: {bad[:40]}')
        sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
