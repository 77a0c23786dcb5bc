"""The two ways a model runs besides training-mode BatchNorm on batch statistics, against the fp32 oracle with torch's own
bf16-autocast run as the noise yardstick (tests/test_engine_host.py):
- eval-mode BatchNorm with gradients on: running statistics, BatchNorm affine frozen (frozen-BN fine-tuning, input gradients
  of an eval model).  The residual unit's ReLU pattern must include the shortcut (engine/functional.py records the mask
  whenever the unit has a ReLU and gradients are on);
- FreezeUnfreeze semantics (train mode, track_running_stats=False, frozen affine): batch statistics, running buffers untouched;
- eval() + no_grad forward of the HRNet segmentation task.
Each test runs on the host stand-in and, marked gpu, through libtok_gfx950.so."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import oracle.hrnet_ref as H
import oracle.torchok_ref as R
import torchok_amd as T
from helpers import cls_config, copy_state, deterministic_state, rel_err
from torchok_amd.constructor.config import apply_schema


@pytest.fixture(params=['host', pytest.param('hip', marks=pytest.mark.gpu)])
def dev(request):
    if request.param == 'host':
        request.getfixturevalue('fake_backend')
        return 'cpu'
    assert torch.cuda.is_available()
    return 'cuda'


IN_CH = 8     # an 8-channel image enters a region without a copy and the stem has a data gradient: the input gradient is the engine's


def seg_config(backbone, classes, size):
    return apply_schema({
        'task': {'name': 'SegmentationTask',
                 'params': {'backbone_name': backbone, 'backbone_params': {'pretrained': False, 'in_channels': IN_CH},
                            'neck_name': 'HRNetSegmentationNeck', 'head_name': 'SegmentationHead',
                            'head_params': {'num_classes': classes},
                            'inputs': [{'shape': [IN_CH, size, size], 'dtype': 'float32'}]}},
        'joint_loss': {'losses': [{'name': 'CrossEntropyLoss', 'params': {'ignore_index': 255},
                                   'mapping': {'input': 'prediction', 'target': 'target'}}]},
        'optimization': [{'optimizer': {'name': 'SGD', 'params': {'lr': 0.01, 'momentum': 0.9}}}],
        'data': {}, 'trainer': {'precision': 'bf16'}})


def _pair(arch, seed):
    """(build task, fp32 oracle, number of classes) on the same deterministic state (non-trivial running statistics)."""
    if arch.startswith('hrnet'):
        classes = 5
        cfg = seg_config(arch, classes, 64)
        task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
        ora = H.SegmentationModel(arch, classes)
        ora.backbone = H.HRNet(arch, in_channels=IN_CH)
    else:
        classes = 10
        cfg = cls_config(arch, classes, backbone_params={'in_channels': IN_CH}, inputs_shape=(IN_CH, 64, 64))
        task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
        ora = R.ClassificationModel(arch, classes, in_channels=IN_CH)
    ora.load_state_dict(deterministic_state(ora.state_dict(), seed))
    copy_state(ora, task)
    return task, ora, classes


def _batch(arch, classes, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(4, IN_CH, 64, 64, generator=g).to(torch.bfloat16).float()    # bf16-exact: every side sees one image
    y = torch.randint(0, classes, (4, 64, 64) if arch.startswith('hrnet') else (4,), generator=g)
    return x, y


def _bn_mode(model, eval_stats: bool):
    """eval_stats: eval() (running statistics); otherwise FreezeUnfreeze's train mode with track_running_stats=False.
    The BatchNorm affine is frozen either way."""
    model.eval() if eval_stats else model.train()
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.weight.requires_grad_(False)
            m.bias.requires_grad_(False)
            if not eval_stats:
                m.track_running_stats = False


def _oracle_grads(ora, x, y, autocast: bool):
    m = copy.deepcopy(ora)
    xi = x.clone().requires_grad_(True)
    with torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
        pred = m.forward_with_gt({'image': xi, 'target': y})['prediction']
    F.cross_entropy(pred.float(), y, ignore_index=255).backward()
    out = {'input': xi.grad}
    out.update({n: p.grad for n, p in m.named_parameters() if p.requires_grad})
    return out, m


def _engine_grads(task, x, y, dev):
    xi = x.to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out = task.forward_with_gt({'image': xi, 'target': y.to(dev)})
    task.losses(**out)[0].backward()
    res = {'input': xi.grad}
    res.update({n: p.grad for n, p in task.named_parameters() if p.requires_grad})
    return res


def _compare(got, g32, gac):
    """Per-tensor distances to the fp32 oracle: (engine, autocast) arrays over the same tensor names."""
    assert set(got) == set(g32) == set(gac)
    names = sorted(g32)
    for n in names:
        assert got[n] is not None and got[n].shape == g32[n].shape, n
    errs = np.array([rel_err(got[n].float(), g32[n]) for n in names])
    yard = np.array([rel_err(gac[n], g32[n]) for n in names])
    return names, errs, yard


EVAL_ARCHS = ['resnet18', 'resnet50', 'hrnet_w18_small', 'hrnet_w18_small_v2']


@pytest.mark.parametrize('arch', EVAL_ARCHS)
def test_eval_bn_gradients_match_oracle(dev, arch):
    """Eval-mode BatchNorm, frozen affine: the input gradient and every conv / fc weight gradient against the fp32 oracle.
    Every residual unit (BasicBlock conv2, Bottleneck conv3, HRNet BasicBlocks) runs its apply pass on running-statistics
    coefficients; in HRNet the fuse rows' deferred terms go through tok_fuse_sum_affine_relu_fwd and the neck runs in the
    direct order.  Recomputing the ReLU pattern without the shortcut put the median error at ~1.0 (autocast: 0.07-0.09)."""
    task, ora, classes = _pair(arch, seed=21)
    _bn_mode(task, True)
    _bn_mode(ora, True)
    x, y = _batch(arch, classes, seed=22)
    g32, _ = _oracle_grads(ora, x, y, autocast=False)
    gac, _ = _oracle_grads(ora, x, y, autocast=True)
    task.to(dev)
    got = _engine_grads(task, x, y, dev)
    names, errs, yard = _compare(got, g32, gac)
    assert 'input' in names and len(names) > 10
    assert np.median(errs) <= 1.5 * np.median(yard) + 1e-2, (np.median(errs), np.median(yard))
    worst = int(np.argmax(errs / yard))
    assert (errs <= 3 * yard).all(), (names[worst], errs[worst], yard[worst])
    # running statistics are read, never written
    want = dict(ora.named_buffers())
    for n, b in task.named_buffers():
        if 'running' in n or 'num_batches' in n:
            assert torch.equal(b.cpu(), want[n]), n


def test_freeze_unfreeze_bn_gradients_match_oracle(dev):
    """FreezeUnfreeze (reference callbacks/freeze_unfreeze.py): train mode, track_running_stats=False, frozen affine —
    batch statistics in forward and backward, the running buffers bit-unchanged.  Must stay distinct from eval mode."""
    arch = 'resnet18'
    task, ora, classes = _pair(arch, seed=23)
    _bn_mode(task, False)
    _bn_mode(ora, False)
    before = {n: b.clone() for n, b in task.named_buffers() if 'running' in n or 'num_batches' in n}
    x, y = _batch(arch, classes, seed=24)
    g32, _ = _oracle_grads(ora, x, y, autocast=False)
    gac, _ = _oracle_grads(ora, x, y, autocast=True)
    task.to(dev)
    got = _engine_grads(task, x, y, dev)
    names, errs, yard = _compare(got, g32, gac)
    assert np.median(errs) <= 1.5 * np.median(yard) + 1e-2, (np.median(errs), np.median(yard))
    worst = int(np.argmax(errs / yard))
    assert (errs <= 3 * yard).all(), (names[worst], errs[worst], yard[worst])
    after = dict(task.named_buffers())
    for n, b in before.items():
        assert torch.equal(after[n].cpu(), b), n


def test_eval_bn_with_trainable_affine_is_refused(dev):
    """Gradients of BatchNorm affine parameters in eval mode are not built: the backward raises instead of returning
    something."""
    task, _, classes = _pair('resnet18', seed=25)
    task.eval().to(dev)
    x, y = _batch('resnet18', classes, seed=26)
    out = task.forward_with_gt({'image': x.to(dev), 'target': y.to(dev)})
    with pytest.raises(NotImplementedError, match='eval mode'):
        task.losses(**out)[0].backward()


@pytest.mark.parametrize('arch', ['hrnet_w18_small', 'hrnet_w18_small_v2'])
def test_hrnet_seg_eval_no_grad_predictions_match_oracle(dev, arch):
    """eval() + no_grad: the segmentation task's predictions against the fp32 oracle and its bf16-autocast run."""
    task, ora, classes = _pair(arch, seed=27)
    task.eval().to(dev)
    ora.eval()
    x, y = _batch(arch, classes, seed=28)
    with torch.no_grad():
        got = task(x.to(dev)).float().cpu()
        want = ora.forward_with_gt({'image': x, 'target': y})['prediction']
        with torch.autocast('cpu', dtype=torch.bfloat16):
            ac = ora.forward_with_gt({'image': x, 'target': y})['prediction'].float()
    assert got.shape == want.shape == (4, classes, 64, 64)
    assert rel_err(got, want) <= 1.5 * rel_err(ac, want) + 1e-2, (rel_err(got, want), rel_err(ac, want))
    assert (got.argmax(1) == want.argmax(1)).float().mean() > 0.95
    assert all(int(m.num_batches_tracked) == 0 for m in task.modules() if isinstance(m, nn.BatchNorm2d))


def test_deferred_affine_is_refused_outside_fuse_sum(fake_backend):
    """A unit with defer_apply hands on its RAW conv output with `.affine = (scale, shift)`: only resample.fuse_sum_relu
    applies those; every other consumer (await_ready, conv_bn_act, bilinear_concat, Region.output) refuses the tensor
    instead of reading un-normalised values."""
    from torchok_amd.engine import core as EC
    from torchok_amd.engine import functional as EF
    from torchok_amd.engine import resample as ER
    torch.manual_seed(0)
    conv, bn = nn.Conv2d(8, 16, 1, bias=False), nn.BatchNorm2d(16)
    conv2, bn2 = nn.Conv2d(16, 16, 1, bias=False), nn.BatchNorm2d(16)
    for m in (conv, bn, conv2, bn2):
        m.eval()
    with torch.no_grad():
        r = EC.Region()
        x = r.input(torch.randn(2, 8, 4, 4).to(torch.bfloat16).contiguous(memory_format=torch.channels_last))
        t = EF.conv_bn_act(r, x, conv, bn, relu=False, defer_apply=True)
        assert t.affine is not None
        with pytest.raises(RuntimeError, match='deferred BatchNorm apply'):
            EC.await_ready(t)
        with pytest.raises(RuntimeError, match='deferred BatchNorm apply'):
            EF.conv_bn_act(r, t, conv2, bn2, relu=True)
        with pytest.raises(RuntimeError, match='deferred BatchNorm apply'):
            ER.bilinear_concat(r, [t], (8, 8))
        with pytest.raises(RuntimeError, match='deferred BatchNorm apply'):
            r.output(t)
        # the consumer that applies it: relu(bn(conv(x))) as the undeferred unit computes it
        got = ER.fuse_sum_relu(r, [(t, 0)], relu=True)
        want = EF.conv_bn_act(r, x, conv, bn, relu=True)
        assert torch.equal(got.data, want.data)
        r.output(got)
