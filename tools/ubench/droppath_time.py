"""Stochastic depth on one MI355X: the tok_bn_droppath_* trio next to the plain launches it replaces in a residual unit
(tok_bn_act_fwd with shortcut and mask / tok_bn_bwd_reduce / tok_bn_bwd_apply with dshortcut) at the four residual shapes of
ResNet-50 at batch 256 (m = B*56*56, c = 256; B*28*28, 512; B*14*14, 1024; B*7*7, 2048), and the resnet50 training step (SGD,
224 x 224) with drop_path_rate 0.0 and 0.1.  The six launches of a shape are timed in alternating windows, several rounds each;
the median is the figure and the spread of the PLAIN launch's rounds (max - min) is the margin a difference has to be read against.
The row scale holds 0 for one sample in ten and 1 / 0.9 for the others.
  python tools/ubench/droppath_time.py [--batch 256] [--size 224] [--steps 20] [--warmup 5] [--rates 0.0 0.1]
                                       [--kernels-only | --step-only]"""
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
    slower = []
    for name, hw, c in [('layer1', 56 * 56, 256), ('layer2', 28 * 28, 512), ('layer3', 14 * 14, 1024), ('layer4', 7 * 7, 2048)]:
        m = batch * hw
        y, sc, dout = (torch.randn(m, c, device='cuda').to(BF) for _ in range(3))
        out, dy, ds = torch.empty_like(y), torch.empty_like(y), torch.empty_like(y)
        mask = torch.empty((m, c // 8), dtype=torch.uint8, device='cuda')
        scale, shift = 0.5 + torch.rand(c, device='cuda'), 0.5 * torch.randn(c, device='cuda')
        mean, rstd = 0.3 * torch.randn(c, device='cuda'), 0.5 + torch.rand(c, device='cuda')
        coef = torch.randn(3, c, device='cuda')
        s = torch.full((batch,), 1 / 0.9, device='cuda')
        s[::10] = 0.0
        partial = torch.empty((2, lib.tok_bn_bwd_rows(m, c), c), device='cuda')
        fwd_b, red_b, app_b = 6 * m * c + m * c // 8, 4 * m * c + m * c // 8, 8 * m * c + m * c // 8
        launches = {
            'fwd    plain    (tok_bn_act_fwd)': (
                lambda: lib.tok_bn_act_fwd(p_(y), p_(scale), p_(shift), p_(sc), 1, p_(out), p_(mask), m, c, st), fwd_b),
            'fwd    droppath (tok_bn_droppath_fwd)': (
                lambda: lib.tok_bn_droppath_fwd(p_(y), p_(scale), p_(shift), p_(sc), p_(s), hw, p_(out), p_(mask), m, c, st), fwd_b),
            'reduce plain    (tok_bn_bwd_reduce)': (
                lambda: lib.tok_bn_bwd_reduce(p_(dout), p_(y), p_(mask), p_(scale), p_(shift), p_(mean), p_(rstd), 1, m, c,
                                              p_(partial), st), red_b),
            'reduce droppath (tok_bn_droppath_bwd_reduce)': (
                lambda: lib.tok_bn_droppath_bwd_reduce(p_(dout), p_(y), p_(mask), p_(s), hw, p_(mean), p_(rstd), m, c, p_(partial),
                                                       st), red_b),
            'apply  plain    (tok_bn_bwd_apply)': (
                lambda: lib.tok_bn_bwd_apply(p_(dout), p_(y), p_(mask), p_(scale), p_(shift), p_(coef), 1, p_(dy), p_(ds), 0, m, c,
                                             st), app_b),
            'apply  droppath (tok_bn_droppath_bwd_apply)': (
                lambda: lib.tok_bn_droppath_bwd_apply(p_(dout), p_(y), p_(mask), p_(s), hw, p_(coef), p_(dy), p_(ds), 0, m, c, st),
                app_b),
        }
        for fn, _ in launches.values():          # warm-up: code objects loaded, every buffer touched, the mask written
            for _ in range(5):
                assert fn() == 0
        torch.cuda.synchronize()
        times = {k: [] for k in launches}
        for _ in range(rounds):                  # alternating windows: drift of the box hits all six alike
            for k, (fn, _) in launches.items():
                times[k].append(_window(fn, reps))
        keys = list(launches)
        for plain, drop in zip(keys[0::2], keys[1::2]):
            tp, td = times[plain], times[drop]
            mp, md = statistics.median(tp), statistics.median(td)
            margin = max(tp) - min(tp)
            for k, t, med in ((plain, tp, mp), (drop, td, md)):
                print(f'{name} ({m} x {c}) {k:46s} median {med:8.1f} us  min {min(t):8.1f}  max {max(t):8.1f}  '
                      f'{launches[k][1] / med / 1e3:6.0f} GB/s  ({rounds} rounds x {reps} launches)')
            verdict = 'within' if md - mp <= margin else 'SLOWER than'
            print(f'{name} {drop.split()[0]:6s} droppath - plain = {md - mp:+.1f} us ({(md / mp - 1) * 100:+.1f} %): {verdict} the plain '
                  f'launch\'s spread of {margin:.1f} us')
            if md - mp > margin:
                slower.append(f'{name} {drop.split()[0]}')
    print(f'launches slower than the plain one by more than its spread: {len(slower)} {slower if slower else ""}')


def step(batch, size, steps, warmup, rate):
    import torchok_amd as T
    from helpers import cls_config
    torch.manual_seed(0)
    params = {'drop_path_rate': rate} if rate is not None else {}
    cfg = cls_config('resnet50', 1000, backbone_params=params, inputs_shape=(3, size, size))
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
    what = 'without the argument' if rate is None else f'drop_path_rate={rate}'
    print(f'resnet50 {what} SGD B={batch} {size}^2: {ms:.2f} ms/step, {batch / ms * 1e3:.0f} img/s, loss {float(loss.detach()):.4f}')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rates', type=float, nargs='*', default=[0.0, 0.1])
    ap.add_argument('--no-argument', action='store_true', help='time the network built without drop_path_rate (any commit)')
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--step-only', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    if not a.step_only:
        kernels(a.batch)
    if not a.kernels_only:
        if a.no_argument:
            step(a.batch, a.size, a.steps, a.warmup, None)
        for r in a.rates:
            step(a.batch, a.size, a.steps, a.warmup, r)
