"""Vision Transformers on one MI355X: the training step (AdamW, 224 x 224, batch 256 by default) of vit_small_patch16_224 and
vit_base_patch16_224 in ms/step and img/s, and the global-attention launches alone at N = 197 / 577 / 785 tokens (224/16,
384/16, 224/8) in us per launch and TF/s (forward 4 N^2 d, backward 10 N^2 d flops per (image, head): the delta pre-pass is
included in the backward), next to torch's scaled_dot_product_attention on the same shapes (reporting only).  The step's
attention share is the isolated launch times of its shape times the layer count over the step time.  bench.py cannot take
this backbone unchanged (it builds its CPU baseline from oracle/), hence this script.
  python tools/ubench/vit_time.py [--batch 256] [--steps 20] [--warmup 5] [--kernels-only | --step-only]"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

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


def attention(batch, heads, n):
    """(fwd us, bwd us) of one attention unit of B images x `heads` heads x n tokens; prints a line with sdpa alongside."""
    from torchok_amd import _C
    lib = _C.lib()
    st = torch.cuda.current_stream().cuda_stream
    p_ = lambda t: t.data_ptr()     # noqa: E731
    c = heads * 64
    qkv = torch.randn(batch * n, 3 * c, device='cuda').to(BF)
    out = torch.empty(batch * n, c, device='cuda', dtype=BF)
    lse = torch.empty(batch, heads, n, device='cuda')
    dout = torch.randn_like(out)
    dqkv = torch.empty_like(qkv)
    wsb = lib.tok_global_attn_bwd_ws_bytes(batch, n, heads)
    ws = torch.empty(wsb // 4, device='cuda')
    t_f = _time(lambda: lib.tok_global_attn_fwd(p_(qkv), 3 * c, batch, n, heads, 64, p_(out), c, p_(lse), st))
    t_b = _time(lambda: lib.tok_global_attn_bwd(p_(qkv), 3 * c, p_(out), p_(dout), c, p_(lse), batch, n, heads, 64, p_(dqkv),
                                                3 * c, p_(ws), wsb, st))
    fl = batch * heads * n * n * 64.0
    q, k, v = (t.detach().requires_grad_(True) for t in
               qkv.view(batch, n, 3, heads, 64).permute(2, 0, 3, 1, 4).contiguous().unbind(0))
    t_sf = _time(lambda: F.scaled_dot_product_attention(q, k, v))
    o = F.scaled_dot_product_attention(q, k, v)
    g = torch.randn_like(o)
    t_sb = _time(lambda: torch.autograd.grad(o, (q, k, v), g, retain_graph=True))
    print(f'attention B={batch} H={heads} N={n:4d}: fwd {t_f:8.1f} us {4 * fl / t_f / 1e6:6.1f} TF/s | '
          f'bwd {t_b:8.1f} us {10 * fl / t_b / 1e6:6.1f} TF/s || sdpa fwd {t_sf:8.1f} us, bwd {t_sb:8.1f} us')
    return t_f, t_b


def step(name, batch, steps, warmup):
    import torchok_amd as T
    from test_vit import vit_config
    torch.manual_seed(0)
    cfg = vit_config(name, 1000, optimizer='AdamW', opt_params={'lr': 1e-3, 'weight_decay': 0.05}, side=224)
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
    print(f'{name} AdamW B={batch} 224^2: {ms:.2f} ms/step, {batch / ms * 1e3:.0f} img/s, loss {float(loss.detach()):.4f}')
    return ms


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--step-only', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    per_layer = {}
    if not a.step_only:
        for heads in (6, 12):
            for n in (197, 577, 785):
                per_layer[(heads, n)] = attention(a.batch if n == 197 else max(a.batch // 4, 1), heads, n)
    if not a.kernels_only:
        for name, heads in (('vit_small_patch16_224', 6), ('vit_base_patch16_224', 12)):
            ms = step(name, a.batch, a.steps, a.warmup)
            if (heads, 197) in per_layer:
                f, b = per_layer[(heads, 197)]
                print(f'  attention share of the step: 12 layers x ({f:.0f} + {b:.0f}) us = {12 * (f + b) / 1e3:.2f} ms '
                      f'({12 * (f + b) / 1e3 / ms * 100:.1f} %)')
