"""Time the tiled window-attention family (csrc/window_attn_tiled.hip) alone at the stage 1 / 2 / 3 geometries of
swinv2_base_window12to24_192to384_22kft1k, B = 8: forward, backward and the d(logits) kernel's share, median of ROUNDS rounds of
LAUNCHES launches, each as a fraction of the bf16 MFMA peak, next to GCViT's largest window in profiles/gcvit_kernel_times.txt
(14 x 14 map, window 14, N = 196, 8 heads, B = 128).  Model flops: forward 4 N^2 32 per (image, window, head) (S and P V),
backward 10 N^2 32 (dP, dV, dK, dQ and one S; the recomputation of S and dP in every kernel is not counted).
Usage: python tools/ubench/swin_tiled_time.py [OUT.txt]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from torchok_amd import _C  # noqa: E402

PEAK = 2.5e15            # dense bf16 MFMA flop/s of one MI355X (data sheet)
ROUNDS, LAUNCHES = 5, 10
BF = torch.bfloat16
P = lambda t: None if t is None else t.data_ptr()       # noqa: E731


def timed(fn):
    for _ in range(3):
        assert fn() == 0
    torch.cuda.synchronize()
    ts = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / LAUNCHES * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def step_line(name='swinv2_base_window12to24_192to384_22kft1k', batch=8, res=384, steps=3):
    """training steps of the 384-px model (forward, backward, AdamW), wall time per step after one warm-up step"""
    import time
    import torchok_amd as T
    from torchok_amd.constructor.config import apply_schema
    cfg = apply_schema({
        'task': {'name': 'ClassificationTask',
                 'params': {'backbone_name': name, 'backbone_params': {'pretrained': False, 'in_channels': 3, 'img_size': res},
                            'pooling_name': 'Pooling', 'head_name': 'ClassificationHead', 'head_params': {'num_classes': 1000},
                            'inputs': [{'shape': [3, res, res], 'dtype': 'float32'}]}},
        'joint_loss': {'losses': [{'name': 'CrossEntropyLoss', 'mapping': {'input': 'prediction', 'target': 'target'}}]},
        'optimization': [{'optimizer': {'name': 'AdamW', 'params': {'lr': 1e-4, 'weight_decay': 0.05}}}],
        'data': {}, 'trainer': {'precision': 'bf16'}})
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params).cuda().train()
    opt = task.configure_optimizers()[0]['optimizer']
    batch_ = {'image': torch.randn(batch, 3, res, res, device='cuda'), 'target': torch.randint(0, 1000, (batch,), device='cuda')}
    ts, loss = [], None
    for i in range(steps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = task.training_step(batch_, i)['loss']
        loss.backward()
        opt.step()
        opt.zero_grad()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return f'{name} AdamW B={batch} {res}^2: {statistics.median(ts[1:]) * 1e3:.1f} ms/step, loss {float(loss):.4f}'


def main():
    lib, st = _C.load_library(), torch.cuda.current_stream().cuda_stream
    lines = ['tiled window attention, B = 8, window 24 (N = 576): us per call, median of %d rounds x %d launches (min .. max), '
             'share of the bf16 MFMA peak (%.1f Pflop/s)' % (ROUNDS, LAUNCHES, PEAK / 1e15)]
    b, ws = 8, 24
    for h, heads, shift in ((96, 4, 0), (96, 4, 12), (48, 8, 0), (24, 16, 0)):
        c, n, nw = heads * 32, ws * ws, (h // ws) ** 2
        qkv = torch.randn(b * h * h, 3 * c, device='cuda').to(BF)
        g = torch.randn(b * h * h, c, device='cuda').to(BF)
        ls, bias = torch.full((heads,), 2.3, device='cuda'), torch.randn(heads, n, n, device='cuda')
        mask = torch.zeros(nw, n, n, device='cuda') if shift else None
        out, lse = torch.empty(b * h * h, c, dtype=BF, device='cuda'), torch.empty(b * nw * heads * n, device='cuda')
        rows = lib.tok_window_attn_bwd_rows(b, h, h, heads, ws)
        wsb = int(lib.tok_window_attn_tiled_ws_bytes(b, h, h, heads, ws))
        dq, wbuf = torch.empty(b * h * h, 3 * c, dtype=BF, device='cuda'), torch.empty(wsb, dtype=torch.uint8, device='cuda')
        scr, dsp = torch.empty(rows, heads * n * n, device='cuda'), torch.empty(rows, heads, device='cuda')
        f = lambda: lib.tok_window_attn_fwd(P(qkv), b, h, h, c, heads, ws, shift, 3 * c, P(ls), P(bias), P(mask), P(out), P(lse), st)  # noqa: E731
        bw = lambda: lib.tok_window_attn_tiled_bwd(P(qkv), P(g), b, h, h, c, heads, ws, shift, 3 * c, P(ls), P(bias), P(mask),  # noqa: E731
                                                   P(lse), P(dq), P(scr), P(dsp), P(wbuf), wsb, st)
        units = b * nw * heads
        tf, tb = timed(f), timed(bw)
        ff, fb = 4.0 * n * n * 32 * units, 10.0 * n * n * 32 * units
        lines.append(f'{h:3d}^2 heads {heads:2d} shift {shift:2d} ({rows} scratch rows, {scr.numel() * 4 / 2**20:.0f} MiB): '
                     f'fwd {tf[0]:8.1f} ({tf[1]:.0f}..{tf[2]:.0f}) {100 * ff / (tf[0] * 1e-6) / PEAK:5.2f} %   '
                     f'bwd {tb[0]:8.1f} ({tb[1]:.0f}..{tb[2]:.0f}) {100 * fb / (tb[0] * 1e-6) / PEAK:5.2f} %')
        print(lines[-1], flush=True)
    units, n = 128 * 8, 196
    lines.append('GCViT 14^2 window 14 heads 8 local, B = 128 (profiles/gcvit_kernel_times.txt): fwd 98.9 us %.2f %%   bwd 432.8 us %.2f %%'
                 % (100 * 4.0 * n * n * 32 * units / 98.9e-6 / PEAK, 100 * 10.0 * n * n * 32 * units / 432.8e-6 / PEAK))
    print(lines[-1], flush=True)
    lines.append(step_line())
    print(lines[-1], flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
