#!/usr/bin/env python
"""Bit-for-bit A/B of every entry of the 64-token-tile attention family (attn_global.hip and gc_attn.hip on attn_tile.h) and of
the embedding helpers of vit_embed.hip between two builds of the library: run once per library with --save, the second time
with --cmp.
    tools/ab_lib.sh <parent>
    TOK_LIB=torchok_amd/lib/libtok_ab.so python tools/ubench/attn_family_check.py --save /tmp/af_a.pt
    python tools/ubench/attn_family_check.py --save /tmp/af_b.pt --cmp /tmp/af_a.pt
Inputs are real-valued (randn from a seeded CPU generator: both runs see the same bits, and a changed fp contraction or addition
order shows only on non-dyadic data).  Every output buffer is filled from the same generator before the call and kept whole, so
pad columns, the LSE and the whole workspace (delta and the d(bias) chunk partials) are compared as raw integers too.
--time prints microseconds per call (device events, after warm-up, over at least 0.5 s of calls) of every attention entry at the
shapes of vit_time.py / beit_time.py (B 256, 12 heads, 197 tokens) and gcvit_time.py (the four stages of gcvit_tiny, B 128),
instead of the bit check; --only TEXT keeps the entries whose name contains TEXT (one shape under a profiler)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from torchok_amd import _C  # noqa: E402

BF = torch.bfloat16
DENSE = [(1, 2, 1), (3, 5, 2), (2, 64, 1), (2, 65, 2), (4, 197, 12), (1, 577, 1), (70, 5, 1), (1, 2305, 2)]      # (b, n, heads)
WINDOWED = [(3, 14, 21, 2, 7), (2, 28, 14, 1, 14), (1, 8, 8, 3, 8), (2, 8, 4, 1, 4)]     # tests/test_gc_attn_contract_gpu.py
GC_STAGES = [(56, 7, 2), (28, 7, 4), (14, 14, 8), (7, 7, 16)]                            # gcvit_tiny: (map side, window, heads)
GEN = torch.Generator().manual_seed(20240911)


def randn(*shape, dtype=BF):
    return torch.randn(*shape, generator=GEN).to(dtype).cuda()


def P(t):
    return None if t is None else t.data_ptr()


def ceil4(n):
    return (n + 3) // 4 * 4


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


def dense(r):
    for b, n, heads in DENSE:
        c = heads * 64
        for pad in (0, 1):                                  # row pitches at the minimum / padded past it
            ldq, ldo, ldb = 3 * c + 24 * pad, c + 8 * pad, ceil4(n) + 4 * pad
            qkv, dout = randn(b * n, ldq), randn(b * n, ldo)
            bias = randn(heads, n, ldb, dtype=torch.float32)
            for biased in (0, 1):
                key = f'dense/{b}x{n}x{heads}/pad{pad}/bias{biased}'
                out, lse = randn(b * n, ldo), randn(b, heads, n, dtype=torch.float32)
                if biased:
                    r.call('tok_global_attn_bias_fwd', P(qkv), ldq, P(bias), ldb, b, n, heads, 64, P(out), ldo, P(lse))
                else:
                    r.call('tok_global_attn_fwd', P(qkv), ldq, b, n, heads, 64, P(out), ldo, P(lse))
                r.keep(key + '/fwd', out, lse)
                if not biased:
                    wsb = r.lib.tok_global_attn_bwd_ws_bytes(b, n, heads)
                    dqkv, ws = randn(b * n, ldq), randn(wsb // 4, dtype=torch.float32)
                    r.call('tok_global_attn_bwd', P(qkv), ldq, P(out), P(dout), ldo, P(lse), b, n, heads, 64, P(dqkv), ldq, P(ws), wsb)
                    r.keep(key + '/bwd', dqkv, ws)
                    continue
                wsb = r.lib.tok_global_attn_bias_bwd_ws_bytes(b, n, heads, ldb)
                for mode in ('null', 'write', 'acc'):
                    dqkv, ws = randn(b * n, ldq), randn(wsb // 4, dtype=torch.float32)
                    dbias = None if mode == 'null' else randn(heads, n, ldb, dtype=torch.float32)
                    r.call('tok_global_attn_bias_bwd', P(qkv), ldq, P(out), P(dout), ldo, P(lse), P(bias), ldb, b, n, heads, 64, P(dqkv),
                           ldq, P(dbias), int(mode == 'acc'), P(ws), wsb)
                    r.keep(f'{key}/bwd_{mode}', dqkv, ws, *([] if dbias is None else [dbias]))


def windowed(r):
    for b, h, w, heads, ws_ in WINDOWED:
        c, n, tokens = heads * 32, ws_ * ws_, b * h * w
        nw = (h // ws_) * (w // ws_)
        for glob in (0, 1):
            for pad in (0, 1):
                parts = 2 if glob else 3
                ld, ldg, ldo, ldb = parts * c + 16 * pad, c + 8 * pad, c + 24 * pad, ceil4(n) + 4 * pad
                qkv, dout = randn(tokens, ld), randn(tokens, ldo)
                qg = randn(b * n, ldg) if glob else None
                bias = randn(heads, n, ldb, dtype=torch.float32)
                key = f'gc/{b}x{h}x{w}x{heads}w{ws_}/glob{glob}/pad{pad}'
                out, lse = randn(tokens, ldo), randn(b * nw, heads, n, dtype=torch.float32)
                r.call('tok_gc_attn_fwd', P(qkv), ld, P(qg), ldg, P(bias), ldb, b, h, w, c, heads, ws_, P(out), ldo, P(lse))
                r.keep(key + '/fwd', out, lse)
                for mode in ('null', 'write', 'acc'):
                    wsb = r.lib.tok_gc_attn_bwd_ws_bytes(b, h, w, heads, ws_, glob, int(mode != 'null'))
                    dqkv, wsbuf = randn(tokens, ld), randn(wsb // 4, dtype=torch.float32)
                    dqg = randn(b * n, ldg) if glob else None
                    dbias = None if mode == 'null' else randn(heads, n, ldb, dtype=torch.float32)
                    r.call('tok_gc_attn_bwd', P(qkv), ld, P(qg), ldg, P(bias), ldb, P(out), P(dout), ldo, P(lse), b, h, w, c, heads, ws_,
                           P(dqkv), ld, P(dqg), ldg, P(dbias), int(mode == 'acc'), P(wsbuf), wsb)
                    r.keep(f'{key}/bwd_{mode}', dqkv, wsbuf, *[t for t in (dqg, dbias) if t is not None])


def embedding(r):
    n, h, w, p = 2, 12, 8, 4
    img, rows = randn(n, h, w, 4), randn(n * (h // p) * (w // p), p * p * 4)
    r.call('tok_patch_gather', P(img), n, h, w, p, P(rows))
    r.keep('embed/patch_gather', rows)
    b, patches, d = 3, 6, 24
    patch, dout = randn(b * patches, d), randn(b * (patches + 1), d)
    for has_cls in (0, 1):
        for nec in (0, 1):
            t = patches + has_cls
            pos = randn(patches if nec else t, d, dtype=torch.float32)
            cls = randn(d, dtype=torch.float32) if has_cls else None
            out = randn(b * t, d)
            r.call('tok_vit_embed_fwd', P(patch), P(pos), P(cls), b, patches, d, nec, P(out))
            for acc in (0, 1):
                dpos, dcls = randn(*pos.shape, dtype=torch.float32), (randn(d, dtype=torch.float32) if has_cls else None)
                r.call('tok_vit_embed_bwd', P(dout), b, patches, d, has_cls, nec, P(dpos), acc, P(dcls), acc)
                r.keep(f'embed/vit/cls{has_cls}nec{nec}acc{acc}', out, dpos, *([] if dcls is None else [dcls]))
    b, t, first, count, d = 2, 7, 2, 3, 16
    src, sel = randn(b * t, d), randn(b * count, d)
    r.call('tok_rows_select', P(src), b, t, first, count, d, P(sel), 0, 0)
    r.keep('embed/rows_select/fwd', sel)
    for acc in (0, 1):
        dsrc = randn(b * t, d)
        r.call('tok_rows_select', P(sel), b, t, first, count, d, P(dsrc), 1, acc)
        r.keep(f'embed/rows_select/bwd{acc}', dsrc)


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


def timing(r, only):
    g = torch.Generator(device='cuda').manual_seed(1)
    rn = lambda *s, dtype=BF: torch.randn(*s, device='cuda', generator=g).to(dtype)      # noqa: E731
    res = []

    def timed(name, fn):
        if only in name:
            res.append((name, time_call(fn)))
    b, n, heads = 256, 197, 12
    c, ldb = heads * 64, ceil4(n)
    qkv, dout, bias = rn(b * n, 3 * c), rn(b * n, c), rn(heads, n, ldb, dtype=torch.float32)
    out, lse, dqkv, dbias = rn(b * n, c), rn(b, heads, n, dtype=torch.float32), rn(b * n, 3 * c), rn(heads, n, ldb, dtype=torch.float32)
    wsb = r.lib.tok_global_attn_bias_bwd_ws_bytes(b, n, heads, ldb)
    ws = torch.empty(wsb // 4, device='cuda')
    timed('vit_b16 global_attn_fwd', lambda: r.call('tok_global_attn_fwd', P(qkv), 3 * c, b, n, heads, 64, P(out), c, P(lse)))
    timed('vit_b16 global_attn_bwd', lambda: r.call(
        'tok_global_attn_bwd', P(qkv), 3 * c, P(out), P(dout), c, P(lse), b, n, heads, 64, P(dqkv), 3 * c, P(ws), wsb))
    timed('beit_b16 global_attn_bias_fwd', lambda: r.call(
        'tok_global_attn_bias_fwd', P(qkv), 3 * c, P(bias), ldb, b, n, heads, 64, P(out), c, P(lse)))
    for name, db in (('beit_b16 global_attn_bias_bwd (dq dk dv)', None), ('beit_b16 global_attn_bias_bwd (+ dbias)', dbias)):
        timed(name, lambda: r.call(
            'tok_global_attn_bias_bwd', P(qkv), 3 * c, P(out), P(dout), c, P(lse), P(bias), ldb, b, n, heads, 64, P(dqkv), 3 * c,
            P(db), 0, P(ws), wsb))
    del qkv, dout, bias, out, lse, dqkv, dbias, ws
    b = 128
    for side, ws_, heads in GC_STAGES:
        c, n, tokens = heads * 32, ws_ * ws_, b * side * side
        nw, ldb = (side // ws_) ** 2, ceil4(ws_ * ws_)
        for glob in (0, 1):
            parts = 2 if glob else 3
            qkv, dout, bias = rn(tokens, parts * c), rn(tokens, c), rn(heads, n, ldb, dtype=torch.float32)
            qg = rn(b * n, c) if glob else None
            out, lse = rn(tokens, c), rn(b * nw, heads, n, dtype=torch.float32)
            dqkv, dqg, dbias = rn(tokens, parts * c), (rn(b * n, c) if glob else None), rn(heads, n, ldb, dtype=torch.float32)
            wsb = r.lib.tok_gc_attn_bwd_ws_bytes(b, side, side, heads, ws_, glob, 1)
            ws = torch.empty(wsb // 4, device='cuda')
            tag = f'gcvit {side}^2 w{ws_} h{heads} {"global" if glob else "local"}'
            timed(tag + ' gc_attn_fwd', lambda: r.call(
                'tok_gc_attn_fwd', P(qkv), parts * c, P(qg), c, P(bias), ldb, b, side, side, c, heads, ws_, P(out), c, P(lse)))
            timed(tag + ' gc_attn_bwd', lambda: r.call(
                'tok_gc_attn_bwd', P(qkv), parts * c, P(qg), c, P(bias), ldb, P(out), P(dout), c, P(lse), b, side, side, c, heads, ws_,
                P(dqkv), parts * c, P(dqg), c, P(dbias), 0, P(ws), wsb))
            del qkv, dout, bias, qg, out, lse, dqkv, dqg, dbias, ws
    for name, us in res:
        print(f'{name:48s} {us:10.2f} us', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--save', default=None)
    ap.add_argument('--cmp', default=None)
    ap.add_argument('--time', action='store_true')
    ap.add_argument('--only', default='', help='with --time: the entries whose name contains this')
    args = ap.parse_args()
    r = Run()
    print('library:', _C.LIB_PATH, flush=True)
    if args.time:
        timing(r, args.only)
        return
    assert args.save, '--save FILE (or --time)'
    for family in (dense, windowed, embedding):
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
