"""mobilenetv3_large_100 on one MI355X: the training step (SGD, 224 x 224, batch 256 by default) in ms/step and img/s, and
the hard-swish BatchNorm forward / backward-apply launches next to tok_bn_act_fwd / tok_bn_bwd_apply with relu=1 (mask
written resp. read) at two layers of that network: (B*56*56, 72) and (B*14*14, 672).  The four launches of a shape are timed
in alternating windows, several rounds each; the median is the figure and the spread of the rounds (min .. max) is the noise
any difference has to be read against.  bench.py cannot take this backbone unchanged (it passes zero_init_last and builds
its CPU baseline from oracle/), hence this script.
  python tools/ubench/mobilenetv3_time.py [--batch 256] [--size 224] [--steps 20] [--warmup 5] [--kernels-only | --step-only]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

BF = torch.bfloat16


def _window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / reps


def kernels(batch, rounds=9, reps=40):
    from torchok_amd import _C
    lib = _C.lib()
    st = torch.cuda.current_stream().cuda_stream
    p_ = lambda t: t.data_ptr()     # noqa: E731
    for name, m, c in [('blocks.1.0 expansion', batch * 56 * 56, 72), ('blocks.4.1 expansion', batch * 14 * 14, 672)]:
        y = torch.randn(m, c, device='cuda').to(BF)
        dout = torch.randn(m, c, device='cuda').to(BF)
        out, dy = torch.empty_like(y), torch.empty_like(y)
        mask = torch.empty((m, c // 8), dtype=torch.uint8, device='cuda')
        scale, shift = torch.rand(c, device='cuda') + 0.5, torch.rand(c, device='cuda') * 2 - 1
        coef = torch.randn(3, c, device='cuda')
        launches = {
            'relu   fwd   (tok_bn_act_fwd, mask written)': (
                lambda: lib.tok_bn_act_fwd(p_(y), p_(scale), p_(shift), None, 1, p_(out), p_(mask), m, c, st), 4 * m * c + m * c // 8),
            'hswish fwd   (tok_bn_hswish_fwd)': (
                lambda: lib.tok_bn_hswish_fwd(p_(y), p_(scale), p_(shift), p_(out), m, c, st), 4 * m * c),
            'relu   apply (tok_bn_bwd_apply, mask read)': (
                lambda: lib.tok_bn_bwd_apply(p_(dout), p_(y), p_(mask), p_(scale), p_(shift), p_(coef), 1, p_(dy), None, 0, m, c,
                                             st), 6 * m * c + m * c // 8),
            'hswish apply (tok_bn_hswish_bwd_apply)': (
                lambda: lib.tok_bn_hswish_bwd_apply(p_(dout), p_(y), p_(scale), p_(shift), p_(coef), p_(dy), m, c, st), 6 * m * c),
        }
        for fn, _ in launches.values():          # warm-up: code objects loaded, every buffer touched
            for _ in range(5):
                assert fn() == 0
        torch.cuda.synchronize()
        times = {k: [] for k in launches}
        for _ in range(rounds):                  # alternating windows: drift of the box hits all four alike
            for k, (fn, _) in launches.items():
                times[k].append(_window(fn, reps))
        for k, (_, nbytes) in launches.items():
            t = times[k]
            med = statistics.median(t)
            print(f'{name:22s} ({m} x {c}) {k:46s} median {med:8.1f} us  min {min(t):8.1f}  max {max(t):8.1f}  '
                  f'{nbytes / med / 1e3:6.0f} GB/s  ({rounds} rounds x {reps} launches)')


def step(batch, size, steps, warmup):
    import torchok_amd as T
    from helpers import cls_config
    torch.manual_seed(0)
    cfg = cls_config('mobilenetv3_large_100', 1000, inputs_shape=(3, size, size))
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
    print(f'mobilenetv3_large_100 SGD B={batch} {size}^2: {ms:.2f} ms/step, {batch / ms * 1e3:.0f} img/s, '
          f'loss {float(loss.detach()):.4f}')


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
