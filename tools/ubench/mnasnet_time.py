"""semnasnet_100 on one MI355X: the training step (SGD, 224 x 224, batch 256 by default) in ms/step and img/s, and the new
depthwise / squeeze-excite launches alone at the largest layers of that network (stage 0-1 depthwise units at 112^2 and 56^2,
the first squeeze-excite at 28^2), in us per launch and GB/s of the bytes each launch must move (each tensor read or
written once).  bench.py cannot take this backbone unchanged (it passes zero_init_last and builds its CPU baseline from
oracle/), hence this script.
  python tools/ubench/mnasnet_time.py [--batch 256] [--size 224] [--steps 20] [--warmup 5] [--kernels-only | --step-only]"""
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


def kernels(batch):
    from torchok_amd import _C
    lib = _C.lib()
    st = torch.cuda.current_stream().cuda_stream
    p_ = lambda t: t.data_ptr()     # noqa: E731
    # (name, c, h, k, stride): the depthwise units of semnasnet_100 at 224^2 with the most bytes
    for name, c, h, k, s in [('blocks.0.0 dw k3 s1', 32, 112, 3, 1), ('blocks.1.0 dw k3 s2', 96, 112, 3, 2),
                             ('blocks.1.1 dw k3 s1', 144, 56, 3, 1), ('blocks.2.0 dw k5 s2', 144, 56, 5, 2),
                             ('blocks.2.1 dw k5 s1', 120, 28, 5, 1)]:
        x = torch.randn(batch, h, h, c, device='cuda').to(BF)
        w = torch.randn(c, k, k, device='cuda')
        p = (h - 1) // s + 1
        out = torch.empty(batch, p, p, c, device='cuda', dtype=BF)
        rows = lib.tok_dwconv_rows(batch, h, h, c, k, s)
        stats = torch.empty(2, rows, c, device='cuda')
        dx = torch.empty_like(x)
        wsb = lib.tok_dwconv_wgrad_ws_bytes(batch, h, h, c, k, s)
        ws = torch.empty(wsb // 4, device='cuda')
        dw = torch.empty(c, k, k, device='cuda')
        nbytes = (x.numel() + out.numel()) * 2
        t_f = _time(lambda: lib.tok_dwconv_fwd(p_(x), p_(w), batch, h, h, c, c, k, s, p_(out), p_(stats), st))
        t_d = _time(lambda: lib.tok_dwconv_dgrad(p_(out), p_(w), batch, h, h, c, c, k, s, p_(dx), 0, st))
        t_w = _time(lambda: lib.tok_dwconv_wgrad(p_(x), p_(out), batch, h, h, c, c, k, s, p_(dw), 0, p_(ws), wsb, st))
        for what, t in (('fwd+stats', t_f), ('dgrad', t_d), ('wgrad', t_w)):
            print(f'{name:22s} B={batch} {h}^2 c={c:4d} {what:9s} {t:8.1f} us  {nbytes / t / 1e3:7.0f} GB/s')
    for name, c, rd, h in [('blocks.2.0 se', 72, 6, 28), ('blocks.4.0 se', 480, 20, 14), ('blocks.5.1 se', 960, 40, 7)]:
        x = torch.randn(batch, h * h, c, device='cuda').to(BF)
        w1, b1 = torch.randn(rd, c, device='cuda'), torch.randn(rd, device='cuda')
        w2, b2 = torch.randn(c, rd, device='cuda'), torch.randn(c, device='cuda')
        mean, gate = torch.empty(batch, c, device='cuda'), torch.empty(batch, c, device='cuda')
        hid = torch.empty(batch, rd, device='cuda')
        ws = torch.empty(lib.tok_se_ws_floats(batch, h * h, c, rd), device='cuda')
        grads = [torch.empty_like(t) for t in (w1, b1, w2, b2)]
        dx = torch.empty_like(x)
        t_f = _time(lambda: lib.tok_se_fwd(p_(x), batch, h * h, c, c, rd, p_(w1), p_(b1), p_(w2), p_(b2), p_(mean), p_(hid),
                                           p_(gate), p_(ws), st))
        t_b = _time(lambda: lib.tok_se_bwd(p_(x), p_(x), batch, h * h, c, c, rd, p_(w1), p_(w2), p_(mean), p_(hid), p_(gate),
                                           *(p_(g) for g in grads), 0, p_(dx), 0, p_(ws), st))
        nb = x.numel() * 2
        print(f'{name:22s} B={batch} {h}^2 c={c:4d} fwd       {t_f:8.1f} us  {nb / t_f / 1e3:7.0f} GB/s (reads x)')
        print(f'{name:22s} B={batch} {h}^2 c={c:4d} bwd       {t_b:8.1f} us  {4 * nb / t_b / 1e3:7.0f} GB/s (dout, x, dout, dx)')


def step(batch, size, steps, warmup):
    import torchok_amd as T
    from helpers import cls_config
    torch.manual_seed(0)
    cfg = cls_config('semnasnet_100', 1000, inputs_shape=(3, size, size))
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params).cuda().train()
    opt = task.configure_optimizers()[0]['optimizer']
    x = torch.randn(batch, 3, size, size, device='cuda')
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
    print(f'semnasnet_100 SGD B={batch} {size}^2: {ms:.2f} ms/step, {batch / ms * 1e3:.0f} img/s, loss {float(loss.detach()):.4f}')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--step-only', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    if not a.step_only:
        kernels(a.batch)
    if not a.kernels_only:
        step(a.batch, a.size, a.steps, a.warmup)
