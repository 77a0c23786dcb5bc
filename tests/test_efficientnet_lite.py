"""EfficientNet-Lite backbones (torchok_amd/models/backbones/efficientnet.py) on the host-memory stand-in of the library: the
ReLU6 BatchNorm entry points are written here in torch, over the layouts the kernels use.  The depth-multiplier rule of the
arch decoder against known answers, construction, state_dict layout, seeded initial weights, teacher-forced blocks and a
training step against the plain-torch restatement (tests/efficientnet_lite_ref.py), eval mode, feature maps, the U-Net neck on
them, the refusals and the recipe.

Tolerance of the block and step comparisons: the project's yardstick (tests/test_resnet_gpu.py) — every tensor as close to the
fp32 restatement as torch's own bf16-autocast CPU run of it, x1.5 + 1e-2."""
import copy
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import efficientnet_lite_ref as L
import fake_backend as fb
import torchok_amd as T
from helpers import cls_config, copy_state, deterministic_state, rel_err
from test_mnasnet import MnasFake
from test_unet import UnetFake
from torchok_amd import engine
from torchok_amd.engine import functional as EF
from torchok_amd.models.backbones import _efficientnet_blocks as B
from torchok_amd.models.backbones import efficientnet as E

RECIPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'recipes')
BF = torch.bfloat16
F32 = torch.float32
NAMES = sorted(L.NAMES)
# the known answers of the depth and width rules (the published EfficientNet B0-B4 tables)
DEPTHS = {'efficientnet_lite0': [1, 2, 2, 3, 3, 4, 1], 'efficientnet_lite1': [1, 3, 3, 4, 4, 5, 1],
          'efficientnet_lite2': [1, 3, 3, 4, 4, 5, 1], 'efficientnet_lite3': [1, 3, 3, 5, 5, 6, 1],
          'efficientnet_lite4': [1, 4, 4, 6, 6, 8, 1]}
WIDTHS = {'efficientnet_lite0': [16, 24, 40, 80, 112, 192, 320], 'efficientnet_lite1': [16, 24, 40, 80, 112, 192, 320],
          'efficientnet_lite2': [16, 24, 48, 88, 120, 208, 352], 'efficientnet_lite3': [24, 32, 48, 96, 136, 232, 384],
          'efficientnet_lite4': [24, 32, 56, 112, 160, 272, 448]}


class LiteFake(MnasFake, UnetFake):
    """MnasFake (depthwise convolution) and UnetFake (nearest resample) plus tok_bn_relu6_*."""

    @staticmethod
    def _r6_z(y, scale, shift, m, c):
        return fb._t(y, (m, c), BF).float() * fb._t(scale, (c,), F32) + fb._t(shift, (c,), F32)

    @staticmethod
    def _r6_dz(dout, z, m, c):
        return fb._t(dout, (m, c), BF).float() * ((z > 0) & (z < 6))

    def tok_bn_relu6_fwd(self, y, scale, shift, out, m, c, st):
        self.calls.append('bn_relu6_fwd')
        fb._t(out, (m, c), BF).copy_(self._r6_z(y, scale, shift, m, c).clamp(0, 6).to(BF))
        return 0

    def tok_bn_relu6_bwd_reduce(self, dout, y, scale, shift, mean, rstd, m, c, partial, st):
        self.calls.append('bn_relu6_bwd_reduce')
        dz = self._r6_dz(dout, self._r6_z(y, scale, shift, m, c), m, c)
        xhat = (fb._t(y, (m, c), BF).float() - fb._t(mean, (c,), F32)) * fb._t(rstd, (c,), F32)
        p = fb._t(partial, (2, 1, c), F32)
        p[0, 0], p[1, 0] = dz.sum(0), (dz * xhat).sum(0)
        return 0

    def tok_bn_relu6_bwd_apply(self, dout, y, scale, shift, coef, dy, m, c, st):
        self.calls.append('bn_relu6_bwd_apply')
        dz = self._r6_dz(dout, self._r6_z(y, scale, shift, m, c), m, c)
        co = fb._t(coef, (3, c), F32)
        fb._t(dy, (m, c), BF).copy_((co[0] * dz + co[1] * fb._t(y, (m, c), BF).float() + co[2]).to(BF))
        return 0


@pytest.fixture
def lite_backend():
    token = fb.install(LiteFake())
    yield token[0]
    fb.uninstall(token)


def _refuse(what):
    raise NotImplementedError(what)


# ---- the arch decoder -----------------------------------------------------------------------------------------------------
def test_decoder_defaults_keep_the_mnasnet_stage_depths():
    """decode_arch_def with its default arguments: the three MnasNet definitions decode to the block counts they name."""
    want = {'_MNASNET_A1': [1, 2, 3, 4, 2, 3, 1], '_MNASNET_B1': [1, 3, 3, 3, 2, 4, 1], '_MNASNET_SMALL': [1, 1, 2, 4, 3, 3, 1]}
    for arch, depths in want.items():
        stages = B.decode_arch_def(getattr(E, arch), _refuse)
        assert [len(s) for s in stages] == depths, arch
        assert all(len({tuple(sorted(b.items())) for b in s}) == 1 for s in stages)       # one definition per stage, repeated
    a1 = B.decode_arch_def(E._MNASNET_A1, _refuse)
    assert a1[0][0] == dict(block_type='ds', kernel_size=3, out_chs=16, stride=1, relu=False, se_ratio=0., noskip=True)
    assert a1[2][0] == dict(block_type='ir', kernel_size=5, out_chs=40, stride=2, relu=False, se_ratio=0.25, noskip=False,
                            exp_ratio=3.0)


@pytest.mark.parametrize('name', NAMES)
def test_depth_and_width_rules_give_the_known_answers(name):
    assert L.stage_depths(name) == DEPTHS[name] and L.stage_widths(name) == WIDTHS[name]
    stages = B.decode_arch_def(E._EFFICIENTNET_LITE, _refuse, depth_multiplier=L.NAMES[name][1], fix_first_last=True)
    assert [len(s) for s in stages] == DEPTHS[name]
    m = T.BACKBONES.get(name)(pretrained=False, in_channels=3)
    assert [len(s) for s in m.blocks] == DEPTHS[name]
    assert [s[-1].conv_pw.out_channels if i == 0 else s[-1].conv_pwl.out_channels for i, s in enumerate(m.blocks)] == WIDTHS[name]
    assert m.conv_stem.out_channels == 32 and m.conv_head.out_channels == m.out_channels == m.num_features == 1280
    assert type(m).__name__ == 'EfficientNet' and m.act == EF.RELU6
    assert not [mod for mod in m.modules() if type(mod).__name__ == 'SqueezeExcite']


def test_depth_rule_details():
    assert B.scale_stage_depth([2], 1.1) == [3] and B.scale_stage_depth([3], 1.4) == [5] and B.scale_stage_depth([4], 1.8) == [8]
    assert B.scale_stage_depth([1, 1, 2], 1.0) == [1, 1, 2]
    assert B.scale_stage_depth([1, 1, 2], 2.0) == [2, 2, 4]               # handed out back to front
    assert B.scale_stage_depth([1, 3], 1.2) == [1, 4]                     # ceil(4.8) = 5: the last entry takes round(3/4 * 5)
    assert B.scale_stage_depth([3], 0.1) == [1]                           # never below one block
    assert B.scale_stage_depth([3], 1.5, 'round') == [4] and B.scale_stage_depth([3], 1.5) == [5]
    unfixed = B.decode_arch_def(E._EFFICIENTNET_LITE, _refuse, depth_multiplier=1.8)
    assert [len(s) for s in unfixed] == [2, 4, 4, 6, 6, 8, 2]             # without fix_first_last the ends grow too
    with pytest.raises(NotImplementedError):
        B.decode_arch_def(E._EFFICIENTNET_LITE, _refuse, depth_trunc='floor')


def test_the_five_names_are_registered():
    assert T.BACKBONES.list_models('efficientnet_lite*') == NAMES
    for name in ('tf_efficientnet_lite0', 'efficientnet_b0', 'mobilenetv2_100', 'mobilenetv2_140'):
        with pytest.raises(KeyError):
            T.BACKBONES.get(name)


# ---- construction and layout ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_state_dict_and_seeded_weights_match_the_restatement(name):
    torch.manual_seed(7)
    m = T.BACKBONES.get(name)()
    torch.manual_seed(7)
    ref = L.EfficientNetLite(name)
    got, want = m.state_dict(), ref.state_dict()
    assert list(got) == list(want)                                          # timm's key order
    assert {k: tuple(v.shape) for k, v in got.items()} == {k: tuple(v.shape) for k, v in want.items()}
    assert all(torch.equal(got[k], want[k]) for k in want)                  # modules() order: the same draws
    ref.load_state_dict(deterministic_state(want, 9))
    m.load_state_dict(ref.state_dict(), strict=True)
    assert all(torch.equal(v, ref.state_dict()[k]) for k, v in m.state_dict().items())


def test_lite0_layout_features_and_stages():
    m = T.BACKBONES.get('efficientnet_lite0')()
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert sd['conv_stem.weight'] == (32, 3, 3, 3) and sd['blocks.0.0.conv_dw.weight'] == (32, 1, 3, 3)
    assert sd['blocks.0.0.conv_pw.weight'] == (16, 32, 1, 1) and sd['blocks.1.0.conv_pw.weight'] == (96, 16, 1, 1)
    assert sd['blocks.2.0.conv_dw.weight'] == (144, 1, 5, 5) and sd['blocks.6.0.conv_pwl.weight'] == (320, 1152, 1, 1)
    assert sd['conv_head.weight'] == (1280, 320, 1, 1) and sd['bn2.running_var'] == (1280,)
    assert m.blocks[2][0].conv_dw.stride == (2, 2) and m.blocks[2][0].conv_dw.padding == (2, 2)
    assert [blk.has_skip for blk in m.blocks[3]] == [False, True, True] and not m.blocks[0][0].has_skip
    assert all(blk.relu is False and blk.act_kw == dict(relu=False, act='relu6') for stage in m.blocks for blk in stage)
    assert [(f['module'], f['reduction'], f['num_chs']) for f in m.feature_info] == [
        ('blocks.0.0', 2, 16), ('blocks.1.1', 4, 24), ('blocks.2.1', 8, 40), ('blocks.4.2', 16, 112), ('blocks.6.0', 32, 320)]
    assert m.out_encoder_channels == (16, 24, 40, 112, 320)
    assert list(m.get_stages(0)) == [m.conv_stem, m.bn1]
    assert list(m.get_stages(8)[-1]) == [m.conv_head, m.bn2]


def test_goog_init_statistics():
    torch.manual_seed(0)
    m = T.BACKBONES.get('efficientnet_lite0')()
    w = m.blocks[5][1].conv_dw.weight            # fan_out = 5 * 5 * 1152 / 1152 groups
    assert abs(float(w.detach().std()) - (2.0 / 25) ** 0.5) < 0.02
    assert float(m.bn2.weight.detach().min()) == 1.0 and float(m.bn2.bias.detach().abs().sum()) == 0.0


# ---- refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kwargs,exc', [({'drop_path_rate': 0.2}, NotImplementedError), ({'output_stride': 16}, NotImplementedError),
                                        ({'act_layer': nn.SiLU}, NotImplementedError), ({'act_layer': 'silu'}, NotImplementedError),
                                        ({'act_layer': nn.Hardswish}, NotImplementedError),
                                        ({'norm_layer': nn.GroupNorm}, NotImplementedError),
                                        ({'pad_type': 'same'}, NotImplementedError), ({'se_layer': nn.Identity}, NotImplementedError),
                                        ({'bn_tf': True}, NotImplementedError), ({'bn_eps': 1e-3}, NotImplementedError),
                                        ({'bn_momentum': 0.01}, NotImplementedError), ({'pretrained': True}, RuntimeError)])
def test_refusals(kwargs, exc):
    with pytest.raises(exc):
        T.BACKBONES.get('efficientnet_lite0')(**kwargs)


@pytest.mark.parametrize('act_layer,act', [(None, 'relu6'), (nn.ReLU6, 'relu6'), ('relu6', 'relu6'), (nn.ReLU, None),
                                           ('relu', None)])
def test_accepted_activations(act_layer, act):
    kw = {} if act_layer is None else {'act_layer': act_layer}
    assert T.BACKBONES.get('efficientnet_lite0')(**kw).act == act
    assert T.BACKBONES.get('mnasnet_small')(**kw).act == (None if act_layer is None else act)      # MnasNet's default stays ReLU


def test_engine_serves_relu6_where_it_serves_hard_swish(lite_backend):
    conv, bn = nn.Conv2d(8, 8, 1, bias=False), nn.BatchNorm2d(8)
    dw = nn.Conv2d(8, 8, 3, padding=1, groups=8, bias=False)
    with engine.region() as r:
        t = r.input(torch.randn(2, 8, 4, 4))
        for kw in ({'shortcut': t}, {'pool': True, 'relu': True}, {'defer_apply': True}):
            with pytest.raises(NotImplementedError):
                EF.conv_bn_act(r, t, conv, bn, act='relu6', **kw)
        with pytest.raises(NotImplementedError):
            EF.conv_bn_act(r, t, conv, None, act='relu6')
        for bad in ('silu', 'relu', 'ReLU6'):
            with pytest.raises(NotImplementedError):
                EF.conv_bn_act(r, t, conv, bn, act=bad)
            with pytest.raises(NotImplementedError):
                EF.dwconv_bn_act(r, t, dw, bn, act=bad)
        r.output(EF.dwconv_bn_act(r, EF.conv_bn_act(r, t, conv, bn, act=EF.RELU6), dw, bn, act='relu6'))
    assert lite_backend.calls.count('bn_relu6_fwd') == 2 and 'bn_act_fwd' not in lite_backend.calls


# ---- teacher-forced blocks on the stand-in against the restatement --------------------------------------------------------------
BLOCKS = {  # name -> (restatement, build, input channels, output channels, stride)
    'ds_k3': (lambda: L.DepthwiseSeparableConv(32, 16, 3, 1),
              lambda: E.DepthwiseSeparableConv(32, 16, 3, 1, False, 0., False, EF.RELU6), 32, 16, 1),
    'ir_k3_skip': (lambda: L.InvertedResidual(24, 24, 3, 1, 6.0),
                   lambda: E.InvertedResidual(24, 24, 3, 1, False, 6.0, 0., False, EF.RELU6), 24, 24, 1),
    'ir_k5_s2': (lambda: L.InvertedResidual(24, 40, 5, 2, 6.0),
                 lambda: E.InvertedResidual(24, 40, 5, 2, False, 6.0, 0., False, EF.RELU6), 24, 40, 2),
}


def perturbed(block):
    with torch.no_grad():
        for name, prm in block.named_parameters():
            if prm.dim() == 1:
                prm.add_(torch.randn_like(prm) * 0.2 + (0.5 if name.endswith('bn3.weight') else 0.0))
    return block


def block_pair(ref_block, eng_block, x, dout, dev, record=None):
    """teacher-forced: the same bf16 input and output gradient into the restatement (fp32 and bf16 autocast) and the engine
    block on `dev`; output within 1e-2, every gradient within the autocast yardstick, running statistics within 1e-2."""
    eng_block.load_state_dict(ref_block.state_dict())
    eng_block.to(dev).train()
    ref_block.train()
    ac_block = copy.deepcopy(ref_block)
    xa = x.float().requires_grad_()
    with torch.autocast('cpu', dtype=BF):
        ya = ac_block(xa)
    ya.float().backward(dout.float())
    xr = x.float().requires_grad_()
    yr = ref_block(xr)
    yr.backward(dout.float())
    xe = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_()
    with engine.region() as r:
        ye = r.output(eng_block(r.input(xe)))
    ye.backward(dout.to(dev).contiguous(memory_format=torch.channels_last))
    if dev != 'cpu':
        torch.cuda.synchronize()
    assert rel_err(ye, yr) <= 1e-2
    assert rel_err(xe.grad, xr.grad) < 1.5 * rel_err(xa.grad, xr.grad) + 1e-2
    rp, ap = dict(ref_block.named_parameters()), dict(ac_block.named_parameters())
    assert {n for n, _ in eng_block.named_parameters()} == set(rp)
    for name, prm in eng_block.named_parameters():
        mine, yard = rel_err(prm.grad, rp[name].grad), rel_err(ap[name].grad, rp[name].grad)
        if record is not None:
            record(name, mine, yard)
        assert mine < 1.5 * yard + 1e-2, (name, mine, yard)
    rb = dict(ref_block.named_buffers())
    for name, b in eng_block.named_buffers():
        if b.is_floating_point():
            assert rel_err(b, rb[name]) <= 1e-2, name


@pytest.mark.parametrize('what', sorted(BLOCKS))
def test_block_matches_the_restatement(lite_backend, what):
    make_ref, make_eng, cin, cout, s = BLOCKS[what]
    torch.manual_seed(0)
    ref, eng = perturbed(make_ref()), make_eng()
    assert eng.has_skip == ref.has_skip == (what == 'ir_k3_skip')
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, cin, 14, 14, generator=g).to(BF)
    dout = torch.randn(4, cout, 14 // s, 14 // s, generator=g).to(BF)
    block_pair(ref, eng, x, dout, 'cpu')
    calls = lite_backend.calls
    n = 1 if what == 'ds_k3' else 2
    assert calls.count('bn_relu6_fwd') == calls.count('bn_relu6_bwd_reduce') == calls.count('bn_relu6_bwd_apply') == n
    assert calls.count('dwconv_fwd') == calls.count('dwconv_wgrad') == calls.count('dwconv_dgrad') == 1


# ---- a training step on the stand-in against the restatement --------------------------------------------------------------------
def _task(name, classes=10):
    cfg = cls_config(name, classes)
    return T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)


_BACKWARD = ('bn_relu6_bwd_reduce', 'bn_relu6_bwd_apply', 'bn_bwd_apply', 'dwconv_wgrad', 'dwconv_dgrad', 'conv_wgrad', 'conv_dgrad')


def test_training_step_matches_the_restatement(lite_backend):
    import oracle.torchok_ref as R
    name = 'efficientnet_lite0'
    torch.manual_seed(0)
    task = _task(name)
    ref = L.Classifier(name, 10)
    ref.load_state_dict(deterministic_state(ref.state_dict(), 3))
    copy_state(ref, task)
    task.train()
    ref.train()
    g = torch.Generator().manual_seed(1)
    # 8 images: the last two stages see 2 x 2 maps, 32 samples per BatchNorm channel
    x, y = torch.randn(8, 3, 64, 64, generator=g), torch.randint(0, 10, (8,), generator=g)
    ref2 = copy.deepcopy(ref)
    with torch.autocast('cpu', dtype=BF):
        o = ref2.forward_with_gt({'image': x, 'target': y})
    ac_loss = F.cross_entropy(o['prediction'].float(), y)
    ac_loss.backward()
    out = task.training_step({'image': x, 'target': y}, 0)
    out['loss'].backward()
    ref_loss, _ = R.training_step(ref, {'image': x, 'target': y}, None)
    # the loss gate of test_mnasnet_gpu.py: one scalar's autocast distance can be small by chance (7e-4 here, a tenth of one
    # bf16 rounding of a loss of 2.4), so the gate does not go below 2e-2
    assert abs(float(out['loss'].detach()) - float(ref_loss)) < max(2e-2, 1.5 * abs(float(ac_loss.detach()) - float(ref_loss)) + 1e-2)
    # L.grad_scale: what the distances of the analytically zero gradients (the bias of a block's last BatchNorm, which feeds
    # only a 1x1 convolution under a batch-statistics BatchNorm) are relative to
    rp, ap = dict(ref.named_parameters()), dict(ref2.named_parameters())
    assert {n for n, _ in task.named_parameters()} == set(rp)
    for n, p in task.named_parameters():
        scale = L.grad_scale(n, rp)
        mine, yard = L.dist(p.grad, rp[n].grad, scale), L.dist(ap[n].grad, rp[n].grad, scale)
        assert mine < 1.5 * yard + 1e-2, (n, mine, yard)
    rb, ab = dict(ref.named_buffers()), dict(ref2.named_buffers())
    for n, b in task.named_buffers():
        if n in rb and b.is_floating_point():            # the running statistics, on the same yardstick
            mine, yard = rel_err(b, rb[n]), rel_err(ab[n], rb[n])
            assert mine < 1.5 * yard + 1e-2, (n, mine, yard)
    calls = lite_backend.calls
    n_units = 1 + 1 + 2 * 15 + 1                  # the stem, the 'ds' block, two per 'ir' block, the head
    assert calls.count('bn_relu6_fwd') == calls.count('bn_relu6_bwd_reduce') == calls.count('bn_relu6_bwd_apply') == n_units
    assert 'se_fwd' not in calls and 'bn_hswish_fwd' not in calls
    assert not any(c in calls for c in ('conv_fwd_bn_apply', 'bn_gram_finalize', 'bn3_bwd_prepare', 'relu_mask_reduce'))  # unit 3
    assert 'dgrad_bnstats' in calls               # the consumer epilogues still serve the linear projections


def test_eval_mode_and_no_grad_forward(lite_backend):
    task = _task('efficientnet_lite0')
    ref = L.Classifier('efficientnet_lite0', 10)
    ref.load_state_dict(deterministic_state(ref.state_dict(), 5))
    copy_state(ref, task)
    task.eval()
    ref.eval()
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        mine = task.backbone(x).float()
        want = ref.backbone(x)
        with torch.autocast('cpu', dtype=BF):
            auto = ref.backbone(x).float()
        feats = task.backbone.forward_features(x)
        want_feats = ref.backbone.forward_features(x)
    assert rel_err(mine, want) < 1.5 * rel_err(auto, want) + 1e-2
    assert [tuple(f.shape) for f in feats] == [(4, 3, 64, 64), (4, 16, 32, 32), (4, 24, 16, 16), (4, 40, 8, 8), (4, 112, 4, 4),
                                               (4, 320, 2, 2)] == [tuple(f.shape) for f in want_feats]
    assert torch.equal(feats[0], x)
    for a, b in zip(feats[1:], want_feats[1:]):
        assert rel_err(a.float(), b) < 5e-2
    assert 'bn_relu6_fwd' in lite_backend.calls and not [c for c in lite_backend.calls if c in _BACKWARD]
    # grad mode, eval-mode BatchNorm (frozen statistics): the backward runs on coef = (scale, 0, 0)
    for p in task.parameters():
        if p.dim() == 1:
            p.requires_grad_(False)
    del lite_backend.calls[:]
    task.backbone(x).float().square().mean().backward()
    assert 'bn_relu6_bwd_apply' in lite_backend.calls and 'bn_relu6_bwd_reduce' not in lite_backend.calls
    assert task.backbone.conv_stem.weight.grad is not None


def test_unet_neck_runs_on_the_lite0_features(lite_backend):
    backbone = T.BACKBONES.get('efficientnet_lite0')().eval()
    neck = T.NECKS.get('UnetNeck')(backbone.out_encoder_channels).eval()
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        image, out = neck(backbone.forward_features(x))
    assert tuple(image.shape) == (2, 3, 64, 64) and tuple(out.shape) == (2, neck.out_channels, 64, 64)
    assert bool(torch.isfinite(out.float()).all()) and 'nearest_fwd' in lite_backend.calls


# ---- the recipe -----------------------------------------------------------------------------------------------------------------
def test_recipe_through_the_fit_loop(lite_backend):
    from torchok_amd.run import fit
    cfg = T.load_config(os.path.join(RECIPES, 'classification_efficientnet_lite0.yaml'), overrides={'trainer.devices': 1})
    assert cfg.task.params.backbone_name == 'efficientnet_lite0'
    torch.manual_seed(0)
    seen = []
    batches = [{'image': torch.randn(4, 3, 64, 64), 'target': torch.randint(0, 10, (4,))} for _ in range(2)]
    res = fit(cfg, batches=batches, max_steps=2, device='cpu', on_step=lambda i, out: seen.append(float(out['loss'])))
    assert res['steps'] == 2 and len(seen) == 2 and all(v == v for v in seen)
    assert 'bn_relu6_bwd_apply' in lite_backend.calls
