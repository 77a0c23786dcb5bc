"""GCViT on one MI355X.

1. The window-attention pair of csrc/gc_attn.hip alone, forward and backward (with d(bias)), local and global mode, at the four
   stage geometries of gcvit_tiny (B = 128 by default), next to a plain-torch bf16 composition of the same attention on the same
   device in the same process: partition, matmul, bias add, softmax, matmul, reverse, with autograd for the backward.  Every
   figure is the median of `--rounds` rounds of 20 launches, the two sides alternating inside a round.  The gate is one
   inequality: forward + backward summed over the stages, weighted by gcvit_tiny's block counts (3, 4, 19, 5), half of them
   global, must be smaller for the HIP pair than for the composition.  Both sides are checked against each other on the timed
   inputs before anything is timed.
2. The training step (AdamW, 224 x 224) of gcvit_xxtiny and gcvit_tiny in ms/step, and with --share the part of the step's
   device time spent in the new kernels (torch.profiler kernel table of three steps, a run of its own after the timed one).

  python tools/ubench/gcvit_time.py [--batch 128] [--steps 15] [--warmup 5] [--rounds 5] [--kernels-only | --step-only]
                                    [--share] [--out profiles/gcvit_kernel_times.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

BF = torch.bfloat16
STAGES = [(56, 7, 2), (28, 7, 4), (14, 14, 8), (7, 7, 16)]          # (token map side, window, heads) of gcvit_tiny
BLOCKS = (3, 4, 19, 5)
_lines = []


def say(s=''):
    print(s, flush=True)
    _lines.append(s)


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


def _med(v):
    return sorted(v)[len(v) // 2]


def _torch_attention(qkv, qg, bias, b, side, heads, ws):
    """the composition: window_partition, (q * scale) k^T + bias, softmax, @ v, window_reverse, in bf16 as autocast runs them"""
    c, n = heads * 32, ws * ws
    nwx = side // ws
    x = qkv.view(b, nwx, ws, nwx, ws, -1).permute(0, 1, 3, 2, 4, 5).reshape(-1, n, qkv.shape[-1])
    bw = x.shape[0]
    if qg is None:
        q, k, v = x.reshape(bw, n, 3, heads, 32).permute(2, 0, 3, 1, 4).unbind(0)
    else:
        k, v = x.reshape(bw, n, 2, heads, 32).permute(2, 0, 3, 1, 4).unbind(0)
        q = qg.view(b, n, c).repeat(bw // b, 1, 1).reshape(bw, n, heads, 32).permute(0, 2, 1, 3)
    attn = ((q * 32 ** -0.5) @ k.transpose(-2, -1) + bias.unsqueeze(0)).softmax(-1)
    o = (attn @ v).transpose(1, 2).reshape(bw, n, c)
    return o.view(b, nwx, nwx, ws, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(b * side * side, c)


def kernels(batch, rounds):
    from torchok_amd import _C
    lib = _C.load_library()
    st = torch.cuda.current_stream().cuda_stream
    p_ = lambda t: None if t is None else t.data_ptr()     # noqa: E731
    say(f'window attention of gcvit_tiny, B={batch}: us per launch, median of {rounds} rounds x 20 launches (min .. max)')
    say(f'{"map":>5} {"ws":>3} {"heads":>5} {"mode":>6} | {"hip fwd":>22} {"hip bwd":>22} | {"torch fwd":>22} {"torch bwd":>22} | '
        f'fwd x   bwd x   pair x')
    total = {'hip': 0.0, 'torch': 0.0}
    for (side, ws, heads), blocks in zip(STAGES, BLOCKS):
        c, n, tokens = heads * 32, ws * ws, batch * side * side
        nw = (side // ws) ** 2
        ldb = (n + 3) // 4 * 4
        for glob in (False, True):
            parts = 2 if glob else 3
            torch.manual_seed(side + glob)
            qkv = torch.randn(tokens, parts * c, device='cuda').to(BF)
            qg = torch.randn(batch * n, c, device='cuda').to(BF) if glob else None
            dout = torch.randn(tokens, c, device='cuda').to(BF)
            bias_p = torch.zeros(heads, n, ldb, device='cuda')
            bias_p[..., :n] = torch.randn(heads, n, n, device='cuda')
            out = torch.empty(tokens, c, device='cuda', dtype=BF)
            lse = torch.empty(batch * nw, heads, n, device='cuda')
            dqkv, dqg, dbias = torch.empty_like(qkv), (torch.empty_like(qg) if glob else None), torch.empty_like(bias_p)
            wsb = lib.tok_gc_attn_bwd_ws_bytes(batch, side, side, heads, ws, int(glob), 1)
            wsbuf = torch.empty(wsb // 4, device='cuda')

            def hip_fwd():
                return lib.tok_gc_attn_fwd(p_(qkv), parts * c, p_(qg), c, p_(bias_p), ldb, batch, side, side, c, heads, ws, p_(out), c,
                                           p_(lse), st)

            def hip_bwd():
                return lib.tok_gc_attn_bwd(p_(qkv), parts * c, p_(qg), c, p_(bias_p), ldb, p_(out), p_(dout), c, p_(lse), batch, side,
                                           side, c, heads, ws, p_(dqkv), parts * c, p_(dqg), c, p_(dbias), 0, p_(wsbuf), wsb, st)
            assert hip_fwd() == 0 and hip_bwd() == 0
            # the composition, with autograd for the backward: the graph is rebuilt by the forward of each backward timing
            xq = qkv.clone().requires_grad_(True)
            xg = qg.clone().requires_grad_(True) if glob else None
            xb = bias_p[..., :n].to(BF).contiguous().requires_grad_(True)
            leaves = [t for t in (xq, xg, xb) if t is not None]

            def torch_fwd():
                with torch.no_grad():
                    return _torch_attention(qkv, qg, xb, batch, side, heads, ws)

            def torch_fwd_bwd():
                for t in leaves:
                    t.grad = None
                _torch_attention(xq, xg, xb, batch, side, heads, ws).backward(dout)
            # same results on the timed inputs (bf16 composition against the kernel: a few bf16 roundings apart)
            ref = torch_fwd().float()
            err = float((out.float() - ref).norm() / ref.norm())
            torch_fwd_bwd()
            gerr = float((dqkv.float() - xq.grad.float()).norm() / xq.grad.float().norm())
            assert err < 2e-2 and gerr < 5e-2, (side, glob, err, gerr)
            t = {k: [] for k in ('hf', 'hb', 'tf', 'tfb')}
            for _ in range(rounds):
                t['hf'].append(_time(hip_fwd))
                t['tf'].append(_time(torch_fwd))
                t['hb'].append(_time(hip_bwd))
                t['tfb'].append(_time(torch_fwd_bwd))
            hf, hb, tf = _med(t['hf']), _med(t['hb']), _med(t['tf'])
            tb = _med([fb - f for fb, f in zip(t['tfb'], t['tf'])])          # backward alone: (forward + backward) - forward
            fmt = lambda v: f'{_med(v):9.1f} ({min(v):.0f}..{max(v):.0f})'     # noqa: E731
            tbl = [fb - f for fb, f in zip(t['tfb'], t['tf'])]
            say(f'{side:>3}^2 {ws:>3} {heads:>5} {"global" if glob else "local":>6} | {fmt(t["hf"]):>22} {fmt(t["hb"]):>22} | '
                f'{fmt(t["tf"]):>22} {fmt(tbl):>22} | {tf / hf:5.2f}   {tb / hb:5.2f}   {(tf + tb) / (hf + hb):5.2f}'
                f'   (out {err:.1e}, dqkv {gerr:.1e} apart)')
            total['hip'] += blocks / 2 * (hf + hb)
            total['torch'] += blocks / 2 * (tf + tb)
            del xq, xg, xb, leaves
            torch.cuda.empty_cache()
    say(f'weighted by the block counts {BLOCKS}, half of each global: hip {total["hip"] / 1e3:.2f} ms, torch composition '
        f'{total["torch"] / 1e3:.2f} ms per step: x{total["torch"] / total["hip"]:.2f}')
    say('GATE ' + ('met' if total['hip'] < total['torch'] else 'MISSED') + ': the HIP pair\'s weighted sum is '
        + ('below' if total['hip'] < total['torch'] else 'NOT below') + ' the composition\'s')
    return total


def step(name, batch, steps, warmup, share):
    from helpers import cls_config
    import torchok_amd as T
    torch.manual_seed(0)
    cfg = cls_config(name, 1000, optimizer='AdamW', opt_params={'lr': 1e-3, 'weight_decay': 0.05}, inputs_shape=(3, 224, 224))
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params).cuda().train()
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
    say(f'{name} AdamW B={batch} 224^2: {ms:.2f} ms/step, {batch / ms * 1e3:.0f} img/s, loss {float(loss.detach()):.4f}')
    if share:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for i in range(3):
                one(i)
            torch.cuda.synchronize()
        dev = lambda e: getattr(e, 'self_device_time_total', None) or getattr(e, 'self_cuda_time_total', 0)     # noqa: E731
        rows = [(e.key, dev(e)) for e in prof.key_averages()]
        whole = sum(t for _, t in rows)
        mine = {}
        for k, t in rows:
            for tag in ('gc_fwd_kernel', 'gc_dkv_kernel', 'gc_dq_kernel', 'gc_dbias_kernel', 'attn_dbias_fold_kernel', 'gc_delta_kernel',
                        'se_fwd_image_kernel', 'se_bwd_image_kernel'):
                if tag in k:
                    mine[tag] = mine.get(tag, 0) + t
        if whole > 0:
            say(f'  device time in the new kernels: {100 * sum(mine.values()) / whole:.1f} % of the kernel time of a step ('
                + ', '.join(f'{k} {100 * v / whole:.1f}' for k, v in sorted(mine.items(), key=lambda kv: -kv[1])) + ')')
    del task, opt
    torch.cuda.empty_cache()
    return ms


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--steps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--step-only', action='store_true')
    ap.add_argument('--share', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    ok = True
    if not a.step_only:
        tot = kernels(a.batch, a.rounds)
        ok = tot['hip'] < tot['torch']
    if not a.kernels_only:
        for name in ('gcvit_xxtiny', 'gcvit_tiny'):
            step(name, a.batch, a.steps, a.warmup, a.share)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(_lines) + '\n')
    sys.exit(0 if ok else 1)
