#!/usr/bin/env python
"""CrossEntropyLoss + DiceLoss on a SegmentationHead output: the fused Dice (csrc/loss_upsample_dice.hip, nothing full-resolution
but the log-sum-exp) against the materialised route (tok_bilinear_fwd -> tok_dice_fwd / _bwd -> tok_bilinear_bwd, what JointLoss
did for DiceLoss before: `DiceLoss.consumes_lazy_logits = False` restores exactly those launches).  The two routes are timed in
turn, `--rounds` times, so that the spread of each is on the page next to their ratio.
  default    head + CE + Dice, forward + backward, batch 16, 128x128 -> 512x512, 19 and 3 classes
  --recipe   the HRNet-W18 CE + Dice recipe of scale_sanity.py, 512x512, B = 8, ms per training step
  --route fused|materialised   one route only (for a kernel trace)
python tools/ubench/upsample_dice_time.py [--recipe] [--rounds 5] [--iters 20]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torchok_amd as T                                            # noqa: E402
from torchok_amd.constructor.config import apply_schema           # noqa: E402
from torchok_amd.losses.base import JointLoss                     # noqa: E402
from torchok_amd.losses.dice import DiceLoss                      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--recipe', action='store_true')
ap.add_argument('--route', default='')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--iters', type=int, default=20)
a = ap.parse_args()
ROUTES = [r for r in ('materialised', 'fused') if not a.route or r == a.route]


def timed(step):
    """ms per call of `step` on each route, a.rounds windows of a.iters calls, the routes alternating"""
    ms = {r: [] for r in ROUTES}
    for rnd in range(a.rounds + 1):
        for r in ROUTES:
            DiceLoss.consumes_lazy_logits = r == 'fused'
            step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                step()
            e1.record()
            torch.cuda.synchronize()
            if rnd:                                                 # (round 0 warms both routes up)
                ms[r].append(e0.elapsed_time(e1) / a.iters)
    return ms


def report(name, ms):
    for r in ROUTES:
        v = sorted(ms[r])
        print(f'{name} {r:>12}: median {v[len(v) // 2]:.3f} ms  (min {v[0]:.3f}, max {v[-1]:.3f}, {len(v)} windows of {a.iters})')
    if len(ROUTES) == 2:
        med = {r: sorted(ms[r])[len(ms[r]) // 2] for r in ROUTES}
        print(f'{name} fused / materialised = {med["fused"] / med["materialised"]:.3f}')


def head_pair(classes, batch=16, hs=128, hd=512):
    torch.manual_seed(0)
    # (272 input channels: the 270 of the HRNet-W18 neck, rounded to the multiple of 8 a region input needs)
    head = T.HEADS.get('SegmentationHead')(in_channels=272, num_classes=classes).cuda().train()
    joint = JointLoss([T.LOSSES.get('CrossEntropyLoss')(), DiceLoss('multiclass')],
                      [{'input': 'prediction', 'target': 'target'}] * 2, [None, None], [None, None])
    img = torch.zeros(batch, 3, hd, hd, device='cuda')
    feat = torch.randn(batch, 272, hs, hs, device='cuda').to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, classes, (batch, hd, hd), device='cuda')

    def step():
        x = feat.detach().requires_grad_(True)
        for p in head.parameters():
            p.grad = None
        loss, _ = joint(prediction=head([img, x]), target=t)
        loss.backward()
    report(f'head + CE + Dice, {classes:2d} classes, B={batch}, {hs}x{hs} -> {hd}x{hd}:', timed(step))


def recipe():
    g = torch.Generator(device='cuda').manual_seed(0)
    cfg = apply_schema({'data': {}, 'trainer': {'precision': 'bf16'},
                        'optimization': [{'optimizer': {'name': 'SGD', 'params': {'lr': 0.01, 'momentum': 0.9, 'weight_decay': 1e-4}}}],
                        'task': {'name': 'SegmentationTask', 'params': {
                            'backbone_name': 'hrnet_w18', 'backbone_params': {'pretrained': False, 'in_channels': 3},
                            'neck_name': 'HRNetSegmentationNeck', 'head_name': 'SegmentationHead', 'head_params': {'num_classes': 3},
                            'inputs': [{'shape': [3, 512, 512], 'dtype': 'float32'}]}},
                        'joint_loss': {'losses': [{'name': 'CrossEntropyLoss', 'mapping': {'input': 'prediction', 'target': 'target'}},
                                                  {'name': 'DiceLoss', 'params': {'mode': 'multiclass'},
                                                   'mapping': {'input': 'prediction', 'target': 'target'}}]}})
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params).cuda().train()
    opt = task.configure_optimizers()[0]['optimizer']
    batch = {'image': torch.randn(8, 3, 512, 512, generator=g, device='cuda').to(torch.bfloat16),
             'target': torch.randint(0, 3, (8, 512, 512), generator=g, device='cuda')}

    def step():
        out = task.training_step(batch, 0)
        opt.zero_grad(set_to_none=True)
        out['loss'].backward()
        opt.step()
    report('hrnet_w18 + CE + Dice recipe, 512x512, B=8, per step:', timed(step))


if a.recipe:
    recipe()
else:
    head_pair(19)
    head_pair(3)
