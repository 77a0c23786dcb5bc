"""efficientnet_lite0 on one MI355X: the training step (SGD, 224 x 224, batch 256 by default) in ms/step and img/s, and the
three ReLU6 BatchNorm launches (tok_bn_relu6_fwd / _bwd_reduce / _bwd_apply) next to their hard-swish counterparts
(tok_bn_hswish_*: the same kernels with the other activation) at three layers of that network: the stem (B*112*112, 32), the
blocks.4 expansion (B*14*14, 672) and the head (B*7*7, 1280).  The six launches of a shape are timed in alternating windows,
several rounds each; the median is the figure and the spread of the rounds (min .. max) is the noise any difference has to be
read against.  bench.py cannot take this backbone unchanged (it passes zero_init_last and builds its CPU baseline from
oracle/), hence this script.
  python tools/ubench/efflite_time.py [--batch 256] [--size 224] [--steps 20] [--warmup 5] [--kernels-only | --step-only]"""
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


def kernels(batch, rounds=9, reps=100):
    from torchok_amd import _C
    lib = _C.lib()
    st = torch.cuda.current_stream().cuda_stream
    p_ = lambda t: t.data_ptr()     # noqa: E731
    for name, m, c in [('stem', batch * 112 * 112, 32), ('blocks.4 expansion', batch * 14 * 14, 672), ('head', batch * 7 * 7, 1280)]:
        y = torch.randn(m, c, device='cuda').to(BF)
        dout = torch.randn(m, c, device='cuda').to(BF)
        out, dy = torch.empty_like(y), torch.empty_like(y)
        # the inputs of tests/test_relu6_contract_gpu.py: every branch of both derivatives is taken
        scale, shift = 1.0 + 3.0 * torch.rand(c, device='cuda'), 4.0 * torch.rand(c, device='cuda') - 1.0
        mean, rstd = torch.zeros(c, device='cuda'), torch.ones(c, device='cuda')
        coef = torch.randn(3, c, device='cuda')
        partial = torch.empty((2, lib.tok_bn_bwd_rows(m, c), c), device='cuda')
        launches = {}
        for act in ('hswish', 'relu6'):
            fwd, red, app = (getattr(lib, f'tok_bn_{act}_{stage}') for stage in ('fwd', 'bwd_reduce', 'bwd_apply'))
            launches[f'{act:6s} fwd    (tok_bn_{act}_fwd)'] = (
                lambda fwd=fwd: fwd(p_(y), p_(scale), p_(shift), p_(out), m, c, st), 4 * m * c)
            launches[f'{act:6s} reduce (tok_bn_{act}_bwd_reduce)'] = (
                lambda red=red: red(p_(dout), p_(y), p_(scale), p_(shift), p_(mean), p_(rstd), m, c, p_(partial), st), 4 * m * c)
            launches[f'{act:6s} apply  (tok_bn_{act}_bwd_apply)'] = (
                lambda app=app: app(p_(dout), p_(y), p_(scale), p_(shift), p_(coef), p_(dy), m, c, st), 6 * m * c)
        for fn, _ in launches.values():          # warm-up: code objects loaded, every buffer touched
            for _ in range(5):
                assert fn() == 0
        torch.cuda.synchronize()
        times = {k: [] for k in launches}
        for _ in range(rounds):                  # alternating windows: drift of the box hits all six alike
            for k, (fn, _) in launches.items():
                times[k].append(_window(fn, reps))
        for k in sorted(launches, key=lambda k: k.split()[1]):       # the two activations of a stage next to each other
            t, nbytes = times[k], launches[k][1]
            med = statistics.median(t)
            print(f'{name:18s} ({m} x {c}) {k:42s} median {med:8.1f} us  min {min(t):8.1f}  max {max(t):8.1f}  '
                  f'{nbytes / med / 1e3:6.0f} GB/s  ({rounds} rounds x {reps} launches)')


def step(batch, size, steps, warmup):
    import torchok_amd as T
    from helpers import cls_config
    torch.manual_seed(0)
    cfg = cls_config('efficientnet_lite0', 1000, inputs_shape=(3, size, size))
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
    print(f'efficientnet_lite0 SGD B={batch} {size}^2: {ms:.2f} ms/step, {batch / ms * 1e3:.0f} img/s, '
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
