"""One training step of a small SwinV2 with 24 x 24 windows (N = 576 tokens: the tiled window-attention family of
csrc/window_attn_tiled.hip) against oracle/swin_ref.py in fp32, with torch's CPU bf16 autocast as the yardstick: stage 1 is a
48 x 48 map of four windows with a shifted block, stage 2 the 24 x 24 map as one window.  Gates as
tests/test_real_geometry_gpu.py::test_swinv2_t_224_window7_step."""
import copy

import pytest
import torch
import torch.nn as nn

import oracle.swin_ref as S
import torchok_amd as T
from helpers import cls_config, deterministic_state, rel_err
from test_real_geometry_gpu import _grad_gate

pytestmark = pytest.mark.gpu


def test_swinv2_window24_step():
    kw = dict(img_size=192, window_size=24, embed_dim=32, depths=(2, 2), num_heads=(1, 2), drop_path_rate=0.0)
    classes = 10
    cfg = cls_config('swinv2_custom', classes, optimizer='AdamW', opt_params={'lr': 1e-3, 'weight_decay': 0.05},
                     backbone_params=dict(kw, depths=list(kw['depths']), num_heads=list(kw['num_heads'])),
                     inputs_shape=(3, 192, 192))
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
    ref = nn.Module()
    ref.backbone, ref.head = S.SwinV2(**kw), nn.Module()
    ref.head.fc = nn.Linear(64, classes)
    sd = deterministic_state(ref.state_dict(), 67)
    ref.load_state_dict(sd)
    missing = task.load_state_dict(sd, strict=False)
    assert all(k.startswith('input_tensors') for k in missing.missing_keys), missing
    task.cuda().train()
    ref.train()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 192, 192, generator=g).bfloat16().float()
    y = torch.randint(0, classes, (2,), generator=g)

    def ref_step(m, ac):
        m.zero_grad()
        with torch.autocast('cpu', dtype=torch.bfloat16, enabled=ac):
            logits = m.head.fc(m.backbone(x).mean((2, 3)))
        loss = nn.functional.cross_entropy(logits.float(), y)
        loss.backward()
        return logits.detach().float(), float(loss), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    l32, loss32, g32 = ref_step(ref, False)
    lac, lossac, gac = ref_step(copy.deepcopy(ref), True)
    out = task.forward_with_gt({'image': x.cuda(), 'target': y.cuda()})
    loss = task.losses(**out)[0]
    loss.backward()
    torch.cuda.synchronize()
    e_log, y_log = rel_err(out['prediction'].float(), l32), rel_err(lac, l32)
    print(f'[step swinv2 window 24] logits rel err HIP {e_log:.3e} (autocast {y_log:.3e}); loss HIP {float(loss):.5f} '
          f'fp32 {loss32:.5f} autocast {lossac:.5f}')
    assert e_log < max(1e-2, 1.5 * y_log)
    assert abs(float(loss) - loss32) < max(1e-2, 1.5 * abs(lossac - loss32)) * max(1.0, abs(loss32))
    ours = {n: p.grad.detach().float().cpu() for n, p in task.named_parameters() if p.grad is not None}
    assert set(g32) <= set(ours), sorted(set(g32) - set(ours))[:5]
    assert any('cpb_mlp' in n for n in g32) and any('logit_scale' in n for n in g32) and any('q_bias' in n for n in g32)
    _grad_gate('swinv2 window 24', ours, g32, gac)
