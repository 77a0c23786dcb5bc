"""Dilated resnet50 (output stride 16 and 8) on one MI355X.
(a) every phase split / merge launch (csrc/phase.hip) of that network at batch 64, 224 x 224, forward and backward (the backward
    of a split is the merge kernel on the same geometry and the reverse; `+=` is the form a second gradient arrival takes): us
    per launch, TB/s of the bytes it must move (the tensor read once and written once; `+=` reads the destination too), and the
    ratio to a device copy of the same tensor (dst.copy_(src)) timed in the same run.  A launch under 0.8 of the copy is FLAGGED.
    Every time is the median of --groups-of repetition groups, the spread (max - min) beside it.
(b) the training step (SGD) of resnet50 at output stride 32, 16 and 8 in ms/step, and the share of that step the permutation
    launches take: the sum of their stand-alone medians from (a) over the step time (an estimate from stand-alone times, not a
    trace of the step).
  python tools/ubench/dilated_time.py [--batch 64] [--size 224] [--steps 10] [--warmup 3] [--kernels-only | --step-only]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

BF = torch.bfloat16
FLAG = 0.8


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


def launches(batch, size):
    """{output_stride: [(where, kernel of the forward, n, h, w, c)]}: n, h, w as the call sees them (a nested split sees the
    phase images of the first as its batch)"""
    s16, s8 = size // 16, size // 8
    return {
        16: [('layer4.1 input', 'split', batch, s16, s16, 2048), ('layer4 output', 'merge', batch, s16, s16, 2048)],
        8: [('layer3.1 input', 'split', batch, s8, s8, 1024), ('layer4.1 input', 'split', batch * 4, s8 // 2, s8 // 2, 2048),
            ('layer4 output, inner', 'merge', batch * 4, s8 // 2, s8 // 2, 2048), ('layer4 output, outer', 'merge', batch, s8, s8, 2048),
            ('layer3 feature (forward_features only)', 'merge', batch, s8, s8, 1024)],
    }


def kernels(batch, size, groups_of):
    from torchok_amd import _C
    lib = _C.lib()
    st = torch.cuda.current_stream().cuda_stream
    fns = {'split': lib.tok_phase_split, 'merge': lib.tok_phase_merge}
    other = {'split': 'merge', 'merge': 'split'}
    flagged, per_step = [], {}
    for os_, rows in launches(batch, size).items():
        total = 0.0
        for where, kind, n, h, w, c in rows:
            src = torch.randn(n, h, w, c, device='cuda').to(BF)
            dst = torch.empty_like(src)
            nbytes = 2 * src.numel() * 2
            tc, sc = _time(lambda: dst.copy_(src), groups_of=groups_of)
            for what, k, acc in (('forward', kind, 0), ('backward', other[kind], 0), ('backward +=', other[kind], 1)):
                fn = fns[k]
                t, s = _time(lambda: _C.check(fn(src.data_ptr(), n, h, w, c, c, 2, dst.data_ptr(), acc, st), k), groups_of=groups_of)
                moved = nbytes + (src.numel() * 2 if acc else 0)
                ratio = (moved / t) / (nbytes / tc)
                flag = ratio < FLAG
                if flag:
                    flagged.append(f'os{os_} {where} {what}')
                if not acc and 'forward_features' not in where:
                    total += t
                print(f'os{os_:<2d} {where:38s} {what:11s} tok_phase_{k:5s} n={n:3d} {h}x{w} c={c:4d} {t:8.1f} us (spread {s:5.1f}) '
                      f'{moved / t / 1e6:5.2f} TB/s | copy {tc:8.1f} us (spread {sc:5.1f}) {nbytes / tc / 1e6:5.2f} TB/s '
                      f'| rate / copy rate {ratio:5.2f}{"  FLAG (< 0.8)" if flag else ""}')
        per_step[os_] = total
    print(f'launches under {FLAG} of the copy: {len(flagged)}' + (': ' + '; '.join(flagged) if flagged else ''))
    return per_step


def step(output_stride, batch, size, steps, warmup):
    import torchok_amd as T
    from helpers import cls_config
    torch.manual_seed(0)
    cfg = cls_config('resnet50', 1000, inputs_shape=(3, size, size), backbone_params={'output_stride': output_stride})
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
    return e0.elapsed_time(e1) / steps, float(loss.detach())


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--groups-of', type=int, default=5)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--step-only', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    per_step = {} if a.step_only else kernels(a.batch, a.size, a.groups_of)
    if not a.kernels_only:
        for os_ in (32, 16, 8):
            ms, loss = step(os_, a.batch, a.size, a.steps, a.warmup)
            share = f', permutation launches {per_step[os_] / 1e3:.3f} ms = {per_step[os_] / 1e3 / ms * 100:.1f} % of the step' \
                if os_ in per_step else ''
            print(f'resnet50 output_stride={os_:2d} SGD B={a.batch} {a.size}^2: {ms:.2f} ms/step, {a.batch / ms * 1e3:.0f} img/s, '
                  f'loss {loss:.4f}{share}')
