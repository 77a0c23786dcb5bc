"""BEiT on one MI355X: the training step (AdamW, 224 x 224, batch 256 by default) of beit_base_patch16_224 in ms/step and img/s,
and the attention launches of its layer alone (B images x 12 heads x 197 tokens): the biased forward / backward
(tok_global_attn_bias_fwd / _bwd with d(bias), and without it) next to the un-biased entry points on the same shape, in us per
launch, repeated `--rounds` times in alternation so that the spread of each figure is on the page; the relative-position gather
and its transpose and the LayerScale residual of the same layer.  TOK_LIB=<path> runs the un-biased half against another build
of the library (a parent build has no biased entry points: --unbiased-only).
  python tools/ubench/beit_time.py [--batch 256] [--steps 20] [--warmup 5] [--rounds 5] [--kernels-only | --step-only]
                                   [--unbiased-only]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

BF = torch.bfloat16


def _time(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / reps


def _fmt(vals):
    return f'{sorted(vals)[len(vals) // 2]:8.1f} us (min {min(vals):.1f}, max {max(vals):.1f})'


def kernels(batch, heads, n, rounds, unbiased_only):
    import ctypes
    from torchok_amd import _C
    if unbiased_only:           # possibly another build (TOK_LIB) that has the un-biased entry points only
        lib = ctypes.CDLL(_C.LIB_PATH)
        for name in ('tok_global_attn_fwd', 'tok_global_attn_bwd_ws_bytes', 'tok_global_attn_bwd'):
            getattr(lib, name).restype, getattr(lib, name).argtypes = _C.PROTOTYPES[name]
    else:
        lib = _C.load_library()
    st = torch.cuda.current_stream().cuda_stream
    p_ = lambda t: t.data_ptr()     # noqa: E731
    c = heads * 64
    ldb = (n + 3) // 4 * 4
    qkv = torch.randn(batch * n, 3 * c, device='cuda').to(BF)
    out = torch.empty(batch * n, c, device='cuda', dtype=BF)
    lse = torch.empty(batch, heads, n, device='cuda')
    dout = torch.randn_like(out)
    dqkv = torch.empty_like(qkv)
    bias = torch.randn(heads, n, ldb, device='cuda')
    dbias = torch.empty_like(bias)
    wsb0 = lib.tok_global_attn_bwd_ws_bytes(batch, n, heads)
    ws0 = torch.empty(wsb0 // 4, device='cuda')
    runs = {
        'un-biased fwd': lambda: lib.tok_global_attn_fwd(p_(qkv), 3 * c, batch, n, heads, 64, p_(out), c, p_(lse), st),
        'un-biased bwd': lambda: lib.tok_global_attn_bwd(p_(qkv), 3 * c, p_(out), p_(dout), c, p_(lse), batch, n, heads, 64,
                                                         p_(dqkv), 3 * c, p_(ws0), wsb0, st),
    }
    if not unbiased_only:
        wsb = lib.tok_global_attn_bias_bwd_ws_bytes(batch, n, heads, ldb)
        ws = torch.empty(wsb // 4, device='cuda')
        runs['biased fwd'] = lambda: lib.tok_global_attn_bias_fwd(p_(qkv), 3 * c, p_(bias), ldb, batch, n, heads, 64, p_(out), c,
                                                                  p_(lse), st)
        runs['biased bwd (dq dk dv)'] = lambda: lib.tok_global_attn_bias_bwd(
            p_(qkv), 3 * c, p_(out), p_(dout), c, p_(lse), p_(bias), ldb, batch, n, heads, 64, p_(dqkv), 3 * c, None, 0, p_(ws),
            wsb, st)
        runs['biased bwd (+ dbias)'] = lambda: lib.tok_global_attn_bias_bwd(
            p_(qkv), 3 * c, p_(out), p_(dout), c, p_(lse), p_(bias), ldb, batch, n, heads, 64, p_(dqkv), 3 * c, p_(dbias), 0,
            p_(ws), wsb, st)
    for fn in runs.values():
        assert fn() == 0
    times = {k: [] for k in runs}
    for _ in range(rounds):                 # alternate: every round visits every launch once
        for k, fn in runs.items():
            times[k].append(_time(fn))
    print(f'attention B={batch} H={heads} N={n} ({os.environ.get("TOK_LIB") or "this tree"}), median of {rounds} rounds x 20 launches')
    for k, v in times.items():
        print(f'  {k:24s} {_fmt(v)}')
    if unbiased_only:
        return times
    med = lambda k: sorted(times[k])[len(times[k]) // 2]     # noqa: E731
    print(f'  cost of the bias: fwd x{med("biased fwd") / med("un-biased fwd"):.3f}, bwd (dq dk dv) '
          f'x{med("biased bwd (dq dk dv)") / med("un-biased bwd"):.3f}, bwd with dbias x{med("biased bwd (+ dbias)") / med("un-biased bwd"):.3f}')
    g = int(round((n - 1) ** 0.5))
    if g * g + 1 == n:
        from beit_ref import gen_relative_position_index
        index = gen_relative_position_index((g, g)).cuda()
        rows = int(index.max()) + 1
        table = torch.randn(rows, heads, device='cuda')
        dtable = torch.empty_like(table)
        t_g = _time(lambda: lib.tok_relpos_bias_fwd(p_(table), p_(index), heads, n, p_(bias), ldb, st))
        t_t = _time(lambda: lib.tok_relpos_bias_bwd(p_(dbias), ldb, p_(index), heads, n, rows, p_(dtable), 0, st))
        print(f'  relative-position gather {t_g:.1f} us, transpose {t_t:.1f} us')
    x, a = torch.randn(batch * n, c, device='cuda').to(BF), torch.randn(batch * n, c, device='cuda').to(BF)
    o, da = torch.empty_like(x), torch.empty_like(x)
    gamma, dgamma = torch.full((c,), 0.1, device='cuda'), torch.empty(c, device='cuda')
    part = torch.empty(lib.tok_layer_scale_bwd_rows(batch * n, c), c, device='cuda')
    t_f = _time(lambda: lib.tok_layer_scale_fwd(p_(x), p_(a), p_(gamma), None, 0, p_(o), batch * n, c, st))
    t_b = _time(lambda: lib.tok_layer_scale_bwd(p_(x), p_(a), p_(gamma), None, 0, p_(da), 0, p_(dgamma), 0, p_(part), batch * n, c, st))
    gb = batch * n * c * 2 / 1e3
    print(f'  LayerScale residual [{batch * n}][{c}]: fwd {t_f:.1f} us ({3 * gb / t_f:.0f} GB/s), bwd {t_b:.1f} us ({3 * gb / t_b:.0f} GB/s)')
    return times


def step(name, batch, steps, warmup):
    from beit_ref import beit_task
    torch.manual_seed(0)
    task = beit_task(backbone=name, num_classes=1000, optimizer='AdamW', opt_params={'lr': 1e-3, 'weight_decay': 0.05},
                     side=224).cuda().train()
    opt = task.configure_optimizers()[0]['optimizer']
    x = torch.randn(batch, 3, 224, 224, device='cuda')
    y = torch.randint(0, 1000, (batch,), device='cuda')

    def one(i):
        out = task.training_step({'image': x, 'target': y}, i)
        opt.zero_grad(set_to_none=True)
        out['loss'].backward()
        opt.step()
        return out['loss']
    for i in range(warmup):
        one(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        loss = one(i)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    print(f'{name} AdamW B={batch} 224^2: {ms:.2f} ms/step, {batch / ms * 1e3:.0f} img/s, loss {float(loss.detach()):.4f}')
    return ms


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--step-only', action='store_true')
    ap.add_argument('--unbiased-only', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    if not a.step_only:
        kernels(a.batch, 12, 197, a.rounds, a.unbiased_only)
    if not a.kernels_only and not a.unbiased_only:
        step('beit_base_patch16_224', a.batch, a.steps, a.warmup)
