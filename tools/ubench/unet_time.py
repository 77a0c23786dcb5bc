"""U-Net segmentation on ResNet-50 at 512x512 B=16 (resnet50 + UnetNeck, default decoder + SegmentationHead + CE): ms per training
step, the neck's forward and backward alone, and the achieved bytes/s of tok_nearest_fwd/_bwd at every shape the neck launches,
next to tok_bilinear_fwd's same-size exact copy (hs == hd) on the same buffers in the same run.  Device events, warmed up.
Bytes from the shapes: forward = source read + slice written, backward = slice read + source written.
    python tools/ubench/unet_time.py [--batch 16] [--size 512] [--iters 10] [--step-only | --model-only]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torchok_amd as T                                   # noqa: E402
from torchok_amd import _C                                # noqa: E402
from torchok_amd.constructor.config import apply_schema   # noqa: E402
from torchok_amd.engine.core import pad8, stream_ptr      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=16)
ap.add_argument('--size', type=int, default=512)
ap.add_argument('--iters', type=int, default=10)
ap.add_argument('--backbone', default='resnet50')
ap.add_argument('--step-only', action='store_true', help='training steps only (for a kernel-trace run of the step)')
ap.add_argument('--model-only', action='store_true', help='skip the per-kernel table (for a kernel-trace run of the model)')
a = ap.parse_args()
dev, BF = 'cuda:0', torch.bfloat16


def timed(fn, iters=a.iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


cfg = apply_schema({
    'task': {'name': 'SegmentationTask',
             'params': {'backbone_name': a.backbone, 'backbone_params': {'pretrained': False, 'in_channels': 3},
                        'neck_name': 'UnetNeck', 'head_name': 'SegmentationHead', 'head_params': {'num_classes': 19},
                        'inputs': [{'shape': [3, a.size, a.size], 'dtype': 'float32'}]}},
    'joint_loss': {'losses': [{'name': 'CrossEntropyLoss', 'mapping': {'input': 'prediction', 'target': 'target'}}]},
    'optimization': [{'optimizer': {'name': 'SGD', 'params': {'lr': 0.01, 'momentum': 0.9, 'weight_decay': 5e-4}}}],
    'data': {}, 'trainer': {'precision': 'bf16'}})
task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params).to(dev).train()
opt = task.configure_optimizers()[0]['optimizer']
g = torch.Generator().manual_seed(0)
batch = {'image': torch.randn(a.batch, 3, a.size, a.size, generator=g).to(dev),
         'target': torch.randint(0, 19, (a.batch, a.size, a.size), generator=g).to(dev)}


def step():
    out = task.training_step(batch, 0)
    opt.zero_grad(set_to_none=True)
    out['loss'].backward()
    opt.step()


print(f'{a.backbone} + UnetNeck + SegmentationHead + CE, {a.size}x{a.size} B={a.batch}: {timed(step):.3f} ms per training step')
if a.step_only:
    sys.exit(0)

with torch.no_grad():
    feats = task.backbone.forward_features(batch['image'])
feats = [feats[0]] + [f.detach() for f in feats[1:]]
gout = None
t_fwd = t_bwd = 0.0
for it in range(3 + a.iters):                  # forward and backward of one pass timed apart, summed over the timed passes
    ins = [feats[0]] + [f.requires_grad_(True) for f in feats[1:]]
    for f in ins[1:]:
        f.grad = None
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    out = task.neck(ins)[1]
    ev[1].record()
    if gout is None:
        gout = torch.randn(out.shape, generator=g).to(dev).to(BF).to(memory_format=torch.channels_last)
    out.backward(gout)
    ev[2].record()
    torch.cuda.synchronize()
    if it >= 3:
        t_fwd += ev[0].elapsed_time(ev[1]) / a.iters
        t_bwd += ev[1].elapsed_time(ev[2]) / a.iters
print(f'neck alone: forward {t_fwd:.3f} ms, backward {t_bwd:.3f} ms')

if a.model_only:
    sys.exit(0)
# ---- the resample kernels at the neck's shapes ----------------------------------------------------------------------------
lib, st = _C.lib(), stream_ptr()
enc = list(task.backbone.out_encoder_channels)[::-1]
dec = [enc[0]] + [b.conv2.conv.out_channels for b in task.neck.blocks]
h = a.size >> 5
print(f'{"kernel":<18}{"source":>18}{"-> slice of":>22}{"MB":>9}{"us":>9}{"TB/s":>8}{"vs copy":>9}')
for i in range(len(task.neck.blocks)):
    hd = h << (i + 1)
    skip = enc[i + 1] if i + 1 < len(enc) else 0
    ld = pad8(dec[i] + skip)
    dst = torch.zeros((a.batch, hd, hd, ld), dtype=BF, device=dev)
    same = torch.randn((a.batch, hd, hd, ld), generator=g, dtype=torch.float32).to(dev).to(BF)
    for c, off, hs in ((dec[i], 0, hd // 2),) + (((skip, dec[i], hd),) if skip else ()):
        src = same[:, :hs, :hs, :c].contiguous()
        dsrc = torch.empty_like(src)
        mb = 2 * (src.numel() + a.batch * hd * hd * c) / 1e6
        # yardstick: the bilinear entry point's exact copy of a same-size source into the same slice
        cp = same[..., :c].contiguous()
        t_copy = timed(lambda: lib.tok_bilinear_fwd(cp.data_ptr(), a.batch, hd, hd, c, c, dst.data_ptr(), hd, hd, ld, off, st))
        r_copy = 4 * cp.numel() / t_copy / 1e9
        t_f = timed(lambda: lib.tok_nearest_fwd(src.data_ptr(), a.batch, hs, hs, c, c, dst.data_ptr(), hd, hd, ld, off, st))
        t_b = timed(lambda: lib.tok_nearest_bwd(dst.data_ptr(), a.batch, hd, hd, ld, off, dsrc.data_ptr(), hs, hs, c, c, 0, st))
        shape = f'{hs}x{hs}x{c}'
        into = f'{hd}x{hd}x{ld}@{off}'
        print(f'{"bilinear copy":<18}{f"{hd}x{hd}x{c}":>18}{into:>22}{4 * cp.numel() / 1e6:9.1f}{t_copy * 1e3:9.1f}{r_copy:8.2f}{"1.00":>9}')
        for name, t in (('tok_nearest_fwd', t_f), ('tok_nearest_bwd', t_b)):
            rate = mb / t / 1e3
            print(f'{name:<18}{shape:>18}{into:>22}{mb:9.1f}{t * 1e3:9.1f}{rate:8.2f}{rate / r_copy:9.2f}')
