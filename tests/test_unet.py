"""UnetNeck (torchok_amd/models/necks/unet_segmentation.py) on the host-memory stand-in of the library: tok_nearest_fwd/_bwd
are written here in torch from the entry points' index rule.  The neck's forward, input gradients and parameter gradients
against the plain-torch restatement (tests/unet_ref.py) at the shapes of tests/golden/unet_neck.npz and at feature sizes whose
skips have to be resized, the refusals, and the ResNet-18 recipe through the task and the fit loop.

Tolerance: the project's yardstick (tests/test_resnet_gpu.py) — every tensor as close to the fp32 restatement as torch's own
bf16-autocast CPU run of it, x1.5 + 1e-2.  The neck's output sits behind 12 conv-BN-ReLU units; the autocast run is the
measurement of how far bf16 drifts there."""
import copy
import os

import numpy as np
import pytest
import torch

import fake_backend as fb
import torchok_amd as T
import unet_ref as U
from helpers import copy_state, deterministic_state, record_distance, rel_err

RECIPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'recipes')
GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'unet_neck.npz'))
IN_CHANNELS, DECODER = GOLD['in_channels'].tolist(), tuple(GOLD['decoder_channels'].tolist())
BF = torch.bfloat16
# (h, w) of the five feature maps, shallow to deep
FIXTURE_SIZES = [(32, 16), (16, 8), (8, 4), (4, 2), (2, 1)]
ODD_SIZES = [(36, 28), (18, 14), (9, 7), (5, 4), (3, 2)]        # ResNet on a 72 x 56 image: every skip is resized


def nearest_index(s, d):
    """min((int)floorf(y * ((float)s / (float)d)), s - 1) for y < d, in fp32 as the kernel computes it"""
    i = np.floor(np.arange(d, dtype=np.float32) * (np.float32(s) / np.float32(d))).astype(np.int64)
    return torch.from_numpy(np.minimum(i, s - 1))


class UnetFake(fb.FakeTok):
    """FakeTok plus tok_nearest_fwd/_bwd."""

    def tok_nearest_fwd(self, src, n, hs, ws, c, ld_src, dst, hd, wd, ld_dst, ch_off, st):
        self.calls.append('nearest_fwd')
        x = fb._t(src, (n, hs, ws, ld_src), BF)
        o = fb._t(dst, (n, hd, wd, ld_dst), BF)
        o[..., ch_off:ch_off + c] = x[:, nearest_index(hs, hd)][:, :, nearest_index(ws, wd)][..., :c]
        return 0

    def tok_nearest_bwd(self, ddst, n, hd, wd, ld_dst, ch_off, dsrc, hs, ws, c, ld_src, accumulate, st):
        self.calls.append('nearest_bwd')
        g = fb._t(ddst, (n, hd, wd, ld_dst), BF)[..., ch_off:ch_off + c].float()
        d = fb._t(dsrc, (n, hs, ws, ld_src), BF)
        rows = torch.zeros(n, hs, wd, c).index_add_(1, nearest_index(hs, hd), g)
        acc = d[..., :c].float() if accumulate else torch.zeros(n, hs, ws, c)
        d[..., :c] = acc.index_add_(2, nearest_index(ws, wd), rows).to(BF)
        return 0


@pytest.fixture
def unet_backend():
    token = fb.install(fake=UnetFake())
    yield token[0]
    fb.uninstall(token)


def test_fake_index_rule_is_atens():
    for s, d in [(1, 2), (3, 6), (5, 6), (7, 13), (9, 9), (6, 3), (28, 32), (1024, 2048)]:
        want = torch.nn.functional.interpolate(torch.arange(s, dtype=torch.float32).view(1, 1, s, 1), size=(d, 1), mode='nearest')
        assert torch.equal(nearest_index(s, d), want.view(-1).long()), (s, d)


def neck_parity(dev, sizes, test, seed=int(GOLD['seed'])):
    """One teacher-forced training-mode forward + backward of the neck on `dev` against the fp32 restatement, yardstick =
    the restatement under CPU bf16 autocast.  All three runs see the same bf16-representable features and d(out)."""
    neck = T.NECKS.get('UnetNeck')(IN_CHANNELS, decoder_channels=DECODER)
    ref = U.UnetNeck(IN_CHANNELS, DECODER)
    ref.load_state_dict(deterministic_state(ref.state_dict(), seed))
    copy_state(ref, neck)
    neck.to(dev).train()
    ref.train()
    ac = copy.deepcopy(ref)
    g = torch.Generator().manual_seed(seed + 1)
    n = 2
    image = torch.zeros(n, 3, 2 * sizes[0][0], 2 * sizes[0][1])
    feats = [torch.randn(n, c, h, w, generator=g).to(BF).float() for c, (h, w) in zip(IN_CHANNELS, sizes)]
    d_out = torch.randn(n, DECODER[-1], 32 * sizes[-1][0], 32 * sizes[-1][1], generator=g).to(BF).float()

    fr = [f.clone().requires_grad_(True) for f in feats]
    out_r = ref([image] + fr)[1]
    out_r.backward(d_out)
    fa = [f.clone().requires_grad_(True) for f in feats]
    with torch.autocast('cpu', dtype=BF):
        out_a = ac([image] + fa)[1]
    out_a.float().backward(d_out)
    fm = [f.to(dev).to(BF).contiguous(memory_format=torch.channels_last).requires_grad_(True) for f in feats]
    img_m, out_m = neck([image.to(dev)] + fm)
    assert tuple(out_m.shape) == tuple(out_r.shape) and tuple(img_m.shape) == tuple(image.shape)
    out_m.backward(d_out.to(dev).to(BF))

    rows = [('out', out_m, out_a, out_r)]
    rows += [(f'd_feat{i}', fm[i].grad, fa[i].grad, fr[i].grad) for i in range(len(feats))]
    ap, rp = dict(ac.named_parameters()), dict(ref.named_parameters())
    rows += [(k, p.grad, ap[k].grad, rp[k].grad) for k, p in neck.named_parameters()]
    assert {k for k, _ in neck.named_parameters()} == set(rp)
    for name, mine, auto, want in rows:
        assert mine is not None, name
        e, yard = rel_err(mine.float(), want), rel_err(auto.float(), want)
        print(f'{test} {name}: hip_vs_fp32 {e:.4g} autocast_vs_fp32 {yard:.4g}')
        if dev != 'cpu':
            record_distance(test, name, hip_vs_fp32=e, autocast_vs_fp32=yard)
        assert e < 1.5 * yard + 1e-2, (name, e, yard)
    # running statistics: bf16 conv outputs feed the batch variance (the bound of test_resnet_gpu.py)
    rb = dict(ref.named_buffers())
    for k, b in neck.named_buffers():
        if k.endswith('num_batches_tracked'):
            assert int(b) == int(rb[k]) == 1
        else:
            assert rel_err(b, rb[k]) < 5e-2, k
    return neck


@pytest.mark.parametrize('sizes', [FIXTURE_SIZES, ODD_SIZES], ids=['fixture_64x32', 'resized_skips_72x56'])
def test_neck_matches_the_restatement(unet_backend, sizes):
    neck_parity('cpu', sizes, 'test_unet::test_neck_matches_the_restatement')
    # five decoder blocks: one concat each; four of them have a skip, whose gradient is a second transpose
    assert unet_backend.calls.count('nearest_fwd') == 4 * 2 + 1
    assert unet_backend.calls.count('nearest_bwd') == 4 * 2 + 1
    assert 'bilinear_fwd' not in unet_backend.calls


def test_fixture_output_of_the_reference(unet_backend):
    """The same comparison against the reference's own numbers: the features of the fixture, its output and gradients."""
    neck = T.NECKS.get('UnetNeck')(IN_CHANNELS, decoder_channels=DECODER)
    neck.load_state_dict(deterministic_state(neck.state_dict(), int(GOLD['seed'])))
    neck.train()
    ac = U.UnetNeck(IN_CHANNELS, DECODER).train()
    ac.load_state_dict(deterministic_state(ac.state_dict(), int(GOLD['seed'])))
    image = torch.zeros(2, 3, 64, 32)
    d_out = torch.from_numpy(GOLD['d_out'])
    fa = [torch.from_numpy(GOLD[f'feat{i}']).requires_grad_(True) for i in range(5)]
    with torch.autocast('cpu', dtype=BF):
        out_a = ac([image] + fa)[1]
    out_a.float().backward(d_out)
    fm = [torch.from_numpy(GOLD[f'feat{i}']).to(BF).contiguous(memory_format=torch.channels_last).requires_grad_(True) for i in range(5)]
    out_m = neck([image] + fm)[1]
    out_m.backward(d_out.to(BF))
    want = torch.from_numpy(GOLD['out'])
    assert rel_err(out_m.float(), want) < 1.5 * rel_err(out_a.float(), want) + 1e-2
    for i in range(5):
        want = torch.from_numpy(GOLD[f'd_feat{i}'])
        assert rel_err(fm[i].grad.float(), want) < 1.5 * rel_err(fa[i].grad, want) + 1e-2, i
    ap = dict(ac.named_parameters())
    for k, p in neck.named_parameters():
        want = torch.from_numpy(GOLD[f'grad__{k}'])
        assert rel_err(p.grad, want) < 1.5 * rel_err(ap[k].grad, want) + 1e-2, k


def test_eval_mode_and_no_grad_forward(unet_backend):
    neck = T.NECKS.get('UnetNeck')(IN_CHANNELS, decoder_channels=DECODER)
    ref = U.UnetNeck(IN_CHANNELS, DECODER)
    ref.load_state_dict(deterministic_state(ref.state_dict(), 5))
    copy_state(ref, neck)
    neck.eval(), ref.eval()
    g = torch.Generator().manual_seed(6)
    image = torch.zeros(2, 3, 72, 56)
    feats = [torch.randn(2, c, h, w, generator=g).to(BF).float() for c, (h, w) in zip(IN_CHANNELS, ODD_SIZES)]
    with torch.no_grad():
        mine = neck([image] + feats)[1].float()
        want = ref([image] + feats)[1]
        with torch.autocast('cpu', dtype=BF):
            auto = ref([image] + feats)[1].float()
    assert mine.shape == (2, DECODER[-1], 96, 64)
    assert rel_err(mine, want) < 1.5 * rel_err(auto, want) + 1e-2
    assert 'nearest_bwd' not in unet_backend.calls


def test_without_centre_block(unet_backend):
    neck = T.NECKS.get('UnetNeck')(IN_CHANNELS, decoder_channels=DECODER, center=False).eval()
    assert isinstance(neck.center, torch.nn.Identity) and not any(k.startswith('center') for k in neck.state_dict())
    feats = [torch.randn(1, c, h, w) for c, (h, w) in zip(IN_CHANNELS, FIXTURE_SIZES)]
    with torch.no_grad():
        assert neck([torch.zeros(1, 3, 64, 32)] + feats)[1].shape == (1, DECODER[-1], 64, 32)


def test_refusals():
    assert T.NECKS.get('UnetNeck') is not None
    with pytest.raises(NotImplementedError, match='use_attention'):
        T.NECKS.get('UnetNeck')(IN_CHANNELS, use_attention=True)
    with pytest.raises(NotImplementedError, match='activation without BatchNorm'):
        T.NECKS.get('UnetNeck')(IN_CHANNELS, use_batchnorm=False)


def _recipe(**extra):
    os.environ.setdefault('HOME', '/root')
    return T.load_config(os.path.join(RECIPES, 'segmentation_unet_resnet18.yaml'),
                         overrides=dict({'task.params.backbone_params.pretrained': False}, **extra))


def test_segmentation_task_builds_from_the_recipe(unet_backend):
    cfg = _recipe()
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params).train()
    assert type(task.neck).__name__ == 'UnetNeck' and type(task.backbone).__name__ == 'ResNet'
    assert tuple(task.neck.in_channels) == (64, 64, 128, 256, 512) and task.head.classifier.in_channels == 64
    assert len(task.as_module()) == 3
    torch.manual_seed(0)
    batch = {'image': torch.randn(2, 3, 72, 56), 'target': torch.randint(0, 3, (2, 72, 56))}
    out = task.training_step(batch, 0)
    assert torch.isfinite(out['loss'])
    out['loss'].backward()
    assert all(p.grad is not None for p in task.parameters())
    task.eval()
    with torch.no_grad():
        assert task(batch['image']).shape == (2, 3, 72, 56)


def test_recipe_through_the_fit_loop(unet_backend):
    from torchok_amd.run import fit
    cfg = _recipe(**{'trainer.precision': 'bf16', 'trainer.devices': 1})
    torch.manual_seed(0)
    seen = []
    batches = [{'image': torch.randn(2, 3, 64, 64), 'target': torch.randint(0, 3, (2, 64, 64))} for _ in range(2)]
    res = fit(cfg, batches=batches, max_steps=2, device='cpu', on_step=lambda i, out: seen.append(float(out['loss'].detach())))
    assert res['steps'] == 2 and len(seen) == 2 and all(v == v for v in seen)
    assert 'nearest_fwd' in unet_backend.calls and 'nearest_bwd' in unet_backend.calls
