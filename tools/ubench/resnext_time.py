"""resnext50_32x4d on one MI355X: the grouped 3x3 launches (csrc/conv_group.hip) at the five 3x3 shapes of that network (batch
256, 224 x 224 by default) — forward with statistics, data gradient, weight gradient — in us per launch, GB/s of the bytes each
launch must move (each activation read or written once) and the fraction of 8 TB/s that is; next to each, the dense kernel
(tok_conv_fwd / tok_conv_dgrad / tok_conv_wgrad with C = K = width) on the same tensor shape in the same run, which moves
the same activations and does `groups` times the arithmetic: the yardstick of the grouped launch.  Every time is the median of
--groups-of repetition groups; the spread (max - min over the groups) is printed beside it, and a grouped launch MISSES the
yardstick when its median exceeds the dense median by more than the larger of the two spreads.  Then the training step (SGD)
in ms/step and img/s.
  python tools/ubench/resnext_time.py [--batch 256] [--size 224] [--steps 20] [--warmup 5] [--kernels-only | --step-only]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

BF = torch.bfloat16
HBM = 8.0e12            # bytes/s


def _time(fn, reps=10, groups_of=5):
    """(median, spread) in us over `groups_of` groups of `reps` launches"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(groups_of):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000.0 / reps)
    ts.sort()
    return ts[len(ts) // 2], ts[-1] - ts[0]


def kernels(batch, scale, groups_of):
    from torchok_amd import _C
    from torchok_amd.engine import functional as EF
    from torchok_amd.engine import paramgrad as PG
    lib = _C.lib()
    st = torch.cuda.current_stream().cuda_stream
    p_ = lambda t: t.data_ptr()     # noqa: E731
    groups = 32
    misses = []
    # (name, width, h, stride): the 3x3 units of resnext50_32x4d at 224^2
    for name, c, h, s in [('layer1.* conv2 s1', 128, 56, 1), ('layer2.0 conv2 s2', 256, 56, 2), ('layer2.* conv2 s1', 256, 28, 1),
                          ('layer3.* conv2 s1', 512, 14, 1), ('layer4.* conv2 s1', 1024, 7, 1)]:
        h = max(h * scale // 224, 1)
        cg = c // groups
        x = torch.randn(batch, h, h, c, device='cuda').to(BF)
        p = (h - 1) // s + 1
        dout = torch.randn(batch, p, p, c, device='cuda').to(BF)
        out, dx = torch.empty_like(dout), torch.empty_like(x)
        nbytes = (x.numel() + out.numel()) * 2
        # grouped: the fp32 master, channels-last as the model keeps it
        w = (torch.randn(c, cg, 3, 3, device='cuda') * (2.0 / (9 * cg)) ** 0.5).contiguous(memory_format=torch.channels_last)
        rows = lib.tok_gconv_rows(batch, h, h, c, groups, s)
        stats = torch.empty(2, rows, c, device='cuda')
        wsb = lib.tok_gconv_wgrad_ws_bytes(batch, h, h, c, groups, s)
        ws = torch.empty(wsb // 4, device='cuda')
        dw = torch.empty_like(w)
        g_f = _time(lambda: lib.tok_gconv_fwd(p_(x), p_(w), 1, batch, h, h, c, c, groups, s, p_(out), p_(stats), st),
                    groups_of=groups_of)
        g_d = _time(lambda: lib.tok_gconv_dgrad(p_(dout), p_(w), 1, batch, h, h, c, c, groups, s, p_(dx), 0, st),
                    groups_of=groups_of)
        g_w = _time(lambda: lib.tok_gconv_wgrad(p_(x), p_(dout), batch, h, h, c, c, groups, s, p_(dw), 1, 0, p_(ws), wsb, st),
                    groups_of=groups_of)
        # dense twin: C = K = width, the engine's own packs, statistics rows and workspace
        wd_ = torch.nn.Parameter((torch.randn(c, c, 3, 3, device='cuda') * (2.0 / (9 * c)) ** 0.5)
                                 .contiguous(memory_format=torch.channels_last))
        d = _C.ConvDesc(batch, h, h, c, c, 3, 3, p, p, s, 1, 3)
        pk = EF.get_packs(wd_, None, c, d.s_pad, c, want_dgrad=True, refresh=True)
        drows = lib.tok_conv_fwd_stat_rows(d)
        dstats = torch.empty(2, drows, c, device='cuda')
        dwsb = PG.wgrad_plan(d)[2]
        dws = torch.empty(max(dwsb // 4, 1), device='cuda')
        ddw = torch.empty(c, 3, 3, c, device='cuda')
        d_f = _time(lambda: lib.tok_conv_fwd(d, p_(x), p_(pk.fwd), None, p_(out), p_(dstats), st), groups_of=groups_of)
        d_d = _time(lambda: lib.tok_conv_dgrad(d, p_(dout), p_(pk.dgrad), p_(dx), 0, st), groups_of=groups_of)
        d_w = _time(lambda: lib.tok_conv_wgrad(d, p_(x), p_(dout), p_(ddw), c, c, p_(dws), dwsb, 0, st), groups_of=groups_of)
        for what, (tg, sg), (td, sd) in (('fwd+stats', g_f, d_f), ('dgrad', g_d, d_d), ('wgrad', g_w, d_w)):
            bw = nbytes / tg * 1e6
            miss = tg > td + max(sg, sd)
            if miss:
                misses.append(f'{name} {what}')
            print(f'{name:18s} B={batch} {h}^2 c={c:4d} cg={cg:2d} {what:9s} grouped {tg:8.1f} us (spread {sg:5.1f}) '
                  f'{bw / 1e9:6.0f} GB/s {bw / HBM:5.2f} of 8 TB/s | dense {td:8.1f} us (spread {sd:5.1f}) '
                  f'| grouped/dense {tg / td:5.2f}{"  MISS" if miss else ""}')
    print(f'launches slower than their dense twin beyond the spread: {len(misses)} of 15' + (': ' + '; '.join(misses) if misses else ''))


def step(batch, size, steps, warmup):
    import torchok_amd as T
    from helpers import cls_config
    torch.manual_seed(0)
    cfg = cls_config('resnext50_32x4d', 1000, inputs_shape=(3, size, size))
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
    print(f'resnext50_32x4d SGD B={batch} {size}^2: {ms:.2f} ms/step, {batch / ms * 1e3:.0f} img/s, loss {float(loss.detach()):.4f}')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--groups-of', type=int, default=5)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--step-only', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    if not a.step_only:
        kernels(a.batch, a.size, a.groups_of)
    if not a.kernels_only:
        step(a.batch, a.size, a.steps, a.warmup)
