"""UnetNeck on the device: the neck teacher-forced against tests/unet_ref.py, and SegmentationTask (resnet18 + UnetNeck +
SegmentationHead) training steps against unet_ref.SegmentationModel, at an image the encoder halves evenly (64 x 64) and at
one it does not (72 x 56: every skip is resized).  Yardstick of every comparison (tests/test_resnet_gpu.py): as close to the
fp32 CPU run as torch's own bf16-autocast CPU run, x1.5 + 1e-2; the distances are recorded with helpers.record_distance.
At 64 x 64 the neck's output already has the image's size, so the head's bilinear step is the identity: those cases also
check that the fused upsample cross-entropy serves hs == hd.

What the whole-step gate can tell apart: torch's own autocast run is 0.4-0.8 away from fp32 on every gradient below the last
decoder block (so the gate admits a relative error near 1 there) and 0.03 / 0.003 away on the last block and the head, where the
gate is tight.  A larger batch and image (B=8, 128 x 128) or targets that follow the image leave those figures where they are:
it is the depth of the train-mode BatchNorm-ReLU chain in bf16, not the sample count at the head map.  The element-wise checks
of the new kernels are tests/test_nearest_contract_gpu.py; the engine wiring is checked in fp32-accumulating torch by
tests/test_unet.py."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

import torchok_amd as T
import unet_ref as U
from helpers import copy_state, deterministic_state, record_distance, rel_err
from test_unet import FIXTURE_SIZES, ODD_SIZES, RECIPES, neck_parity
from torchok_amd.constructor.config import apply_schema

pytestmark = pytest.mark.gpu
CLASSES, BATCH = 3, 2


@pytest.mark.parametrize('sizes', [FIXTURE_SIZES, ODD_SIZES], ids=['fixture_64x32', 'resized_skips_72x56'])
def test_neck_teacher_forced(sizes):
    neck_parity('cuda', sizes, f'test_unet_gpu::test_neck_teacher_forced[{sizes[0][0] * 2}x{sizes[0][1] * 2}]')


def seg_config(dice):
    losses = [{'name': 'CrossEntropyLoss', 'mapping': {'input': 'prediction', 'target': 'target'}}]
    if dice:
        losses.append({'name': 'DiceLoss', 'params': {'mode': 'multiclass'}, 'mapping': {'input': 'prediction', 'target': 'target'}})
    return apply_schema({
        'task': {'name': 'SegmentationTask',
                 'params': {'backbone_name': 'resnet18', 'backbone_params': {'pretrained': False, 'in_channels': 3},
                            'neck_name': 'UnetNeck', 'head_name': 'SegmentationHead', 'head_params': {'num_classes': CLASSES},
                            'inputs': [{'shape': [3, 64, 64], 'dtype': 'float32'}]}},
        'joint_loss': {'losses': losses},
        'optimization': [{'optimizer': {'name': 'SGD', 'params': {'lr': 0.01, 'momentum': 0.9, 'weight_decay': 5e-4}}}],
        'data': {}, 'trainer': {'precision': 'bf16'}})


def dice_multiclass(logits, target, eps=1e-7):
    """DiceLoss('multiclass') of the reference (losses/segmentation/dice.py) with its defaults: softmax, one-hot, per-class
    score over the whole batch, classes absent from the target masked, mean over classes."""
    c = logits.shape[1]
    p = logits.float().softmax(1).permute(0, 2, 3, 1).reshape(-1, c)
    y = F.one_hot(target.reshape(-1), c).float()
    score = 2 * (p * y).sum(0) / (p.sum(0) + y.sum(0)).clamp_min(eps)
    return ((1 - score) * (y.sum(0) > 0)).mean()


def ref_loss(model, x, y, dice, autocast=False):
    if autocast:
        with torch.autocast('cpu', dtype=torch.bfloat16):
            z = model.forward_with_gt({'image': x, 'target': y})['prediction']
    else:
        z = model.forward_with_gt({'image': x, 'target': y})['prediction']
    ce = F.cross_entropy(z.float(), y)
    return 0.5 * ce + 0.5 * dice_multiclass(z, y) if dice else ce       # JointLoss normalises the two unit weights


def make_pair(dice, seed=21):
    cfg = seg_config(dice)
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
    ref = U.SegmentationModel(CLASSES)
    ref.load_state_dict(deterministic_state(ref.state_dict(), seed))
    copy_state(ref, task)
    return task.cuda().train(), ref.train()


def batch_of(size, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(BATCH, 3, *size, generator=g), torch.randint(0, CLASSES, (BATCH, *size), generator=g)


@pytest.mark.parametrize('dice', [False, True], ids=['ce', 'ce_dice'])
@pytest.mark.parametrize('size', [(64, 64), (72, 56)], ids=['64x64', '72x56'])
def test_training_step_vs_restatement(size, dice):
    test = f'test_unet_gpu::test_training_step_vs_restatement[{size[0]}x{size[1]}-{"ce_dice" if dice else "ce"}]'
    task, ref = make_pair(dice)
    x, y = batch_of(size)
    ac = copy.deepcopy(ref)
    ac_loss = ref_loss(ac, x, y, dice, autocast=True)
    ac_loss.backward()
    out = task.training_step({'image': x.cuda(), 'target': y.cuda()}, 0)
    assert set(out) == {'loss'}
    out['loss'].backward()
    want = ref_loss(ref, x, y, dice)
    want.backward()
    torch.cuda.synchronize()
    got, want, ac_loss = float(out['loss'].detach()), float(want.detach()), float(ac_loss.detach())
    print(f'{test} loss: hip {got:.6f} fp32 {want:.6f} autocast {ac_loss:.6f}')
    record_distance(test, 'loss', hip_vs_fp32=abs(got - want), autocast_vs_fp32=abs(ac_loss - want))
    assert abs(got - want) < max(2e-2, 1.5 * abs(ac_loss - want) + 1e-2)
    rp, ap = dict(ref.named_parameters()), dict(ac.named_parameters())
    assert {n for n, _ in task.named_parameters()} == set(rp)
    failed = []
    for n, p in task.named_parameters():
        assert p.grad is not None, n
        mine, yard = rel_err(p.grad, rp[n].grad), rel_err(ap[n].grad, rp[n].grad)
        print(f'{test} {n}: hip_vs_fp32 {mine:.4g} autocast_vs_fp32 {yard:.4g}')
        record_distance(test, n, hip_vs_fp32=mine, autocast_vs_fp32=yard)
        if not mine < 1.5 * yard + 1e-2:
            failed.append((n, mine, yard))
    assert not failed, failed
    rb = dict(ref.named_buffers())
    for n, b in task.named_buffers():
        if n not in rb:
            continue
        if n.endswith('num_batches_tracked'):
            assert int(b) == int(rb[n]) == 1
        else:
            assert rel_err(b, rb[n]) < 5e-2, n   # bf16 conv outputs feed the batch variance (tests/test_resnet_gpu.py)


@pytest.mark.parametrize('size', [(64, 64), (72, 56)], ids=['64x64', '72x56'])
def test_eval_forward(size):
    task, ref = make_pair(False, seed=5)
    task.eval(), ref.eval()
    x, y = batch_of(size, seed=2)
    with torch.no_grad():
        got = task(x.cuda()).float().cpu()
        want = ref.forward_with_gt({'image': x, 'target': y})['prediction']
        with torch.autocast('cpu', dtype=torch.bfloat16):
            auto = ref.forward_with_gt({'image': x, 'target': y})['prediction'].float()
    assert got.shape == (BATCH, CLASSES, *size)
    mine, yard = rel_err(got, want), rel_err(auto, want)
    record_distance(f'test_unet_gpu::test_eval_forward[{size[0]}x{size[1]}]', 'prediction', hip_vs_fp32=mine, autocast_vs_fp32=yard)
    assert mine < 1.5 * yard + 1e-2, (mine, yard)


def test_two_identical_steps_give_identical_gradients():
    grads = []
    x, y = batch_of((72, 56), seed=3)
    for _ in range(2):
        task, _ref = make_pair(True, seed=9)
        task.training_step({'image': x.cuda(), 'target': y.cuda()}, 0)['loss'].backward()
        torch.cuda.synchronize()
        grads.append({n: p.grad.detach().clone() for n, p in task.named_parameters()})
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]), n


def test_recipe_through_the_fit_loop_on_the_device():
    from torchok_amd.run import fit
    os.environ.setdefault('HOME', '/root')
    cfg = T.load_config(os.path.join(RECIPES, 'segmentation_unet_resnet18.yaml'),
                        overrides={'task.params.backbone_params.pretrained': False, 'trainer.precision': 'bf16',
                                   'trainer.devices': 1})
    torch.manual_seed(0)
    seen = []
    batches = [{'image': torch.randn(2, 3, 64, 64).cuda(), 'target': torch.randint(0, 3, (2, 64, 64)).cuda()} for _ in range(2)]
    res = fit(cfg, batches=batches, max_steps=2, device='cuda:0', on_step=lambda i, out: seen.append(float(out['loss'].detach())))
    assert res['steps'] == 2 and len(seen) == 2 and all(v == v for v in seen)
