"""ecaresnet50d on one MI355X: the ECA residual launches (csrc/eca.hip) on the sixteen block outputs of that network (batch 256,
224 x 224 by default) next to the BatchNorm apply-with-shortcut launch (tok_bn_act_fwd with a shortcut, ReLU and mask: the
pass a plain bottleneck ends with) ON THE SAME TENSORS, then the training step (SGD).

Two ways to read it:
  * as it prints: per stage shape, us per launch from device events (median of --groups-of groups, spread beside it), GB/s of
    the bytes the launch must move and the ratio to the apply launch's GB/s;
  * under `rocprofv3 --kernel-trace --stats -- python tools/ubench/ecaresnet_time.py --trace`: every launch once per block of the
    network (3 + 4 + 6 + 3), so that the per-kernel totals of the trace divide into the byte totals printed at the end.
Bytes a launch must move (bf16 tensors of T bytes): eca sum pass T (forward) / 3 T (backward: dout, out, z), eca out pass 3 T
(z, shortcut, out), eca dz/dshort pass 4 T (dout, out, dz, dshort), apply-with-shortcut 3 T + T / 16 (y, shortcut, out, mask).
  python tools/ubench/ecaresnet_time.py [--batch 256] [--size 224] [--steps 20] [--warmup 5] [--kernels-only | --step-only | --trace]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

BF, F32 = torch.bfloat16, torch.float32
# (stage, blocks, channels, map side at 224, window)
STAGES = [('layer1', 3, 256, 56, 5), ('layer2', 4, 512, 28, 5), ('layer3', 6, 1024, 14, 5), ('layer4', 3, 2048, 7, 7)]


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


class Stage:
    def __init__(self, batch, c, h, k):
        from torchok_amd import _C
        self.lib, self.n, self.hw, self.c, self.k = _C.lib(), batch, h * h, c, k
        mk = lambda: torch.randn(batch, h, h, c, device='cuda').to(BF)      # noqa: E731
        self.z, self.sc, self.dout = mk(), mk(), mk()
        self.out, self.dz, self.ds = (torch.empty_like(self.z) for _ in range(3))
        self.w = torch.randn(k, device='cuda') * 0.4
        self.mean, self.gate = (torch.empty(batch, c, device='cuda') for _ in range(2))
        self.ws = torch.empty(self.lib.tok_eca_ws_floats(batch, self.hw, c), device='cuda')
        self.dw = torch.empty(k, device='cuda')
        self.scale, self.shift = torch.rand(c, device='cuda') + 0.5, torch.randn(c, device='cuda')
        self.mask = torch.empty(batch * self.hw, c // 8, dtype=torch.uint8, device='cuda')
        self.tensor_bytes = self.z.numel() * 2
        self.st = torch.cuda.current_stream().cuda_stream

    def fwd(self):
        p = lambda t: t.data_ptr()     # noqa: E731
        return self.lib.tok_eca_fwd(p(self.z), p(self.sc), self.n, self.hw, self.c, self.c, p(self.w), self.k, p(self.mean),
                                    p(self.gate), p(self.out), p(self.ws), self.st)

    def bwd(self):
        p = lambda t: t.data_ptr()     # noqa: E731
        return self.lib.tok_eca_bwd(p(self.dout), p(self.out), p(self.z), self.n, self.hw, self.c, self.c, p(self.w), self.k,
                                    p(self.mean), p(self.gate), p(self.dw), 0, p(self.dz), 0, p(self.ds), 0, p(self.ws), self.st)

    def apply(self):
        p = lambda t: t.data_ptr()     # noqa: E731
        return self.lib.tok_bn_act_fwd(p(self.z), p(self.scale), p(self.shift), p(self.sc), 1, p(self.dz), p(self.mask),
                                       self.n * self.hw, self.c, self.st)


def kernels(batch, size, groups_of):
    for name, blocks, c, h, k in STAGES:
        s = Stage(batch, c, max(h * size // 224, 1), k)
        assert s.fwd() == 0 and s.bwd() == 0 and s.apply() == 0
        T = s.tensor_bytes
        rows = []
        for what, fn, nbytes in (('eca fwd (sum, image, out)', s.fwd, 4 * T), ('eca bwd (sum, image, dw, dz/dshort)', s.bwd, 7 * T),
                                 ('bn apply + shortcut', s.apply, 3 * T + T // 16)):
            t, sp = _time(fn, groups_of=groups_of)
            rows.append((what, t, sp, nbytes / t * 1e6))
        ref = rows[-1][3]
        for what, t, sp, bw in rows:
            print(f'{name} B={batch} {s.hw:5d} px c={c:4d} k={k} {what:36s} {t:8.1f} us (spread {sp:5.1f}) {bw / 1e9:6.0f} GB/s '
                  f'= {bw / ref:4.2f} of the apply launch')


def trace(batch, size):
    """every launch once per block of the network, then the byte totals its kernels must move"""
    tot = dict(sum_fwd=0, out=0, sum_bwd=0, dx=0, apply=0)
    for name, blocks, c, h, k in STAGES:
        s = Stage(batch, c, max(h * size // 224, 1), k)
        for _ in range(blocks):
            assert s.fwd() == 0 and s.bwd() == 0 and s.apply() == 0
        torch.cuda.synchronize()
        T = s.tensor_bytes * blocks
        for key, f in (('sum_fwd', 1), ('out', 3), ('sum_bwd', 3), ('dx', 4), ('apply', 3 + 1 / 16)):
            tot[key] += T * f
    print('bytes per kernel over the 16 blocks: ' + ', '.join(f'{k} {v / 1e9:.3f} GB' for k, v in tot.items()))


def step(batch, size, steps, warmup):
    import torchok_amd as T
    from helpers import cls_config
    torch.manual_seed(0)
    cfg = cls_config('ecaresnet50d', 1000, inputs_shape=(3, size, size))
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
    print(f'ecaresnet50d SGD B={batch} {size}^2: {ms:.2f} ms/step, {batch / ms * 1e3:.0f} img/s, loss {float(loss.detach()):.4f}')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--groups-of', type=int, default=5)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--step-only', action='store_true')
    ap.add_argument('--trace', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    if a.trace:
        trace(a.batch, a.size)
    else:
        if not a.step_only:
            kernels(a.batch, a.size, a.groups_of)
        if not a.kernels_only:
            step(a.batch, a.size, a.steps, a.warmup)
