"""Dilated ResNets (output_stride 8 / 16): the dilated stages run in phase layout (engine.functional.phase_split / phase_merge,
csrc/phase.hip) on the units of the plain network.  Host side: the host-memory stand-in of the library plus tok_phase_split /
tok_phase_merge written here with torch indexing (and tok_gconv_* of tests/test_resnext.py for the ResNeXt member).  Module
trees against the plain-torch restatement (tests/dilated_ref.py: the oracle's blocks under the reference's stage rule), a phased
convolution unit against the fp64 dilated convolution exactly, training steps inside the bf16 yardstick of the fp32 restatement,
features, eval, no-grad, frozen weights, output_stride=32 bit for bit the default, the refusals, and on the GPU two identical
steps bit for bit and the YAML recipe through the fit loop."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

import dilated_ref as D
import fake_backend as fb
import oracle.torchok_ref as R
import torchok_amd as T
from helpers import cls_config, copy_state, deterministic_state, record_distance, rel_err
from test_resnext import ResNeXtFake
from torchok_amd import engine
from torchok_amd.engine import functional as EF

BF, F32 = torch.bfloat16, torch.float32
RECIPES = os.path.join(os.path.dirname(__file__), 'recipes')


class DilatedFake(ResNeXtFake):
    """FakeTok (+ tok_gconv_*) plus tok_phase_split / tok_phase_merge."""

    @staticmethod
    def _views(merged, phased, n, h, w, c, ld, d):
        served = d in (2, 4) and n >= 1 and h % d == 0 and w % d == 0 and c % 8 == 0 and ld >= c and ld % 8 == 0
        if not served or merged is None or phased is None:
            return None, None
        m = fb._t(merged, (n, h // d, d, w // d, d, ld), BF).permute(0, 2, 4, 1, 3, 5)[..., :c]     # [n][a][b][y][x][k]
        return m, fb._t(phased, (n, d, d, h // d, w // d, ld), BF)[..., :c]

    def tok_phase_split(self, x, n, h, w, c, ld, d, out, accumulate, st):
        self.calls.append('phase_split')
        src, dst = self._views(x, out, n, h, w, c, ld, d)
        if src is None:
            return 1
        dst.copy_((dst.float() + src.float()).to(BF) if accumulate else src)
        return 0

    def tok_phase_merge(self, xs, n, h, w, c, ld, d, out, accumulate, st):
        self.calls.append('phase_merge')
        dst, src = self._views(out, xs, n, h, w, c, ld, d)
        if src is None:
            return 1
        dst.copy_((dst.float() + src.float()).to(BF) if accumulate else src)
        return 0


@pytest.fixture
def dilated_backend():
    token = fb.install(fake=DilatedFake())
    yield token[0]
    fb.uninstall(token)


@pytest.fixture(params=['host', pytest.param('hip', marks=pytest.mark.gpu)])
def dev(request):
    if request.param == 'host':
        request.getfixturevalue('dilated_backend')
        return 'cpu'
    assert torch.cuda.is_available()
    return 'cuda'


def _pair(backbone, output_stride, dev, seed=23, **opt):
    """the task on `dev` and the fp32 restatement with the same deterministic state, both in train mode"""
    cfg = cls_config(backbone, 10, backbone_params={'zero_init_last': False, 'output_stride': output_stride}, **opt)
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
    ref = R.ClassificationModel(D.key(backbone, output_stride), 10, zero_init_last=False)
    ref.load_state_dict(deterministic_state(ref.state_dict(), seed))
    copy_state(ref, task)
    task.to(dev).train()
    ref.train()
    return task, ref


def _autocast_loss(model, x, y):
    with torch.autocast('cpu', dtype=torch.bfloat16):
        o = model.forward_with_gt({'image': x, 'target': y})
    return F.cross_entropy(o['prediction'].float(), y)


# ---- construction ------------------------------------------------------------------------------------------------------------
def _triple(conv):
    assert conv.stride[0] == conv.stride[1] and conv.padding[0] == conv.padding[1] and conv.dilation[0] == conv.dilation[1]
    return conv.stride[0], conv.padding[0], conv.dilation[0]


@pytest.mark.parametrize('name,output_stride', [('resnet18', 8), ('resnet18', 16), ('resnet50', 8), ('resnet50', 16),
                                                ('resnext50_32x4d', 16)])
def test_module_tree_equals_the_restatement(dilated_backend, name, output_stride):
    mine = T.BACKBONES.get(name)(pretrained=False, in_channels=3, output_stride=output_stride)
    ref = D.build(name, output_stride)
    assert [(k, tuple(v.shape)) for k, v in mine.state_dict().items()] == \
        [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    convs = {n: m for n, m in mine.named_modules() if isinstance(m, torch.nn.Conv2d)}
    rconvs = {n: m for n, m in ref.named_modules() if isinstance(m, torch.nn.Conv2d)}
    assert list(convs) == list(rconvs)
    for n, m in convs.items():
        assert (_triple(m), m.groups, m.kernel_size) == (_triple(rconvs[n]), rconvs[n].groups, rconvs[n].kernel_size), n
    for n, want in D.EXPECTED[(name, output_stride)].items():      # ... and the restatement is what the rule says
        assert _triple(convs[n]) == want, (n, _triple(convs[n]), want)
    assert [f['reduction'] for f in mine.feature_info] == D.REDUCTIONS[output_stride]
    assert mine.feature_info == ref.feature_info


# ---- the phased convolution unit against the fp64 dilated convolution, exactly --------------------------------------------------
@pytest.mark.parametrize('steps', [(2,), (4,), (2, 2)])
def test_phased_conv_unit_is_the_dilated_convolution(dev, steps):
    """small integers: every product, sum and stored value is exact in bf16 / fp32, so output, dx and dw must EQUAL fp64"""
    d = 1
    for s in steps:
        d *= s
    g = torch.Generator().manual_seed(5 + d + len(steps))
    n, c, k, h, w = 2, 8, 16, 2 * d, 3 * d
    x = torch.randint(-1, 2, (n, c, h, w), generator=g).float()
    wt = torch.randint(-1, 2, (k, c, 3, 3), generator=g).float()
    gy = torch.randint(-1, 2, (n, k, h, w), generator=g).float()
    conv = torch.nn.Conv2d(c, k, 3, padding=d, dilation=d, bias=False)
    with torch.no_grad():
        conv.weight.copy_(wt)
    conv = conv.to(memory_format=torch.channels_last).to(dev)
    xin = x.to(BF).contiguous(memory_format=torch.channels_last).to(dev).requires_grad_(True)
    with engine.region() as r:
        t = r.input(xin)
        for s in steps:
            t = EF.phase_split(r, t, s)
        assert t.phase == d and t.phase_steps == steps and t.shape == (n * d * d, h // d, w // d, c)
        y = EF.conv_bn_act(r, t, conv, None)
        assert y.phase == d and y.phase_steps == steps
        with pytest.raises(RuntimeError, match='phase layout'):
            r.output(y)
        out = r.output(EF.from_phase(r, y))
    out.backward(gy.to(BF).contiguous(memory_format=torch.channels_last).to(dev))
    x64 = x.double().requires_grad_(True)
    w64 = wt.double().requires_grad_(True)
    ref = F.conv2d(x64, w64, padding=d, dilation=d)
    ref.backward(gy.double())
    assert torch.equal(out.detach().double().cpu(), ref.detach())
    assert torch.equal(xin.grad.double().cpu(), x64.grad)
    assert torch.equal(conv.weight.grad.double().cpu(), w64.grad)


def test_phase_rules_of_the_units(dilated_backend):
    conv3 = lambda d, **kw: torch.nn.Conv2d(8, 8, 3, padding=d, dilation=d, bias=False, **kw)      # noqa: E731
    bn = torch.nn.BatchNorm2d(8)
    with engine.region() as r:
        t = r.input(torch.randn(1, 8, 8, 8))
        assert t.phase == 1 and t.phase_steps == () and EF.to_phase(r, t, 1) is t
        # today's message for a dilation the tensor's phase does not match, at phase 1 and in phase layout
        with pytest.raises(NotImplementedError, match='dilation == 1 and groups == 1'):
            EF.conv_bn_act(r, t, conv3(2), bn, relu=True)
        t2 = EF.to_phase(r, t, 2)
        assert t2.phase == 2 and EF.to_phase(r, t2, 2) is t2
        with pytest.raises(NotImplementedError, match='dilation == 1 and groups == 1'):
            EF.conv_bn_act(r, t2, conv3(4), bn, relu=True)
        t4 = EF.to_phase(r, t2, 4)
        assert t4.phase == 4 and t4.phase_steps == (2, 2) and t4.shape == (16, 2, 2, 8)
        with pytest.raises(ValueError):
            EF.to_phase(r, t4, 2)                                  # never merges implicitly
        with pytest.raises(ValueError):
            EF.phase_merge(r, t4, 4)                               # the last split was by 2
        assert EF.phase_merge(r, t4, 2).phase_steps == (2,)
        assert EF.from_phase(r, t4).phase == 1
        # everything that is not phase-agnostic refuses a phased tensor
        for bad in (lambda: EF.conv_bn_act(r, t2, conv3(1), bn, relu=True),                          # a plain 3x3
                    lambda: EF.conv_bn_act(r, t2, torch.nn.Conv2d(8, 8, 1, stride=2, bias=False), bn),   # strided
                    lambda: EF.subsample2(r, t2), lambda: EF.max_pool_3x3_s2(r, t2), lambda: EF.avg_pool_2x2(r, t2),
                    lambda: EF.global_avg_pool(r, t2), lambda: EF.global_pool(r, t2, 'max'),
                    lambda: EF.eca_residual(r, t2, None, t2), lambda: r.output(t2)):
            with pytest.raises(RuntimeError, match='phase layout'):
                bad()
        # a shortcut must be in the unit's phase layout
        with pytest.raises((RuntimeError, ValueError)):
            EF.conv_bn_act(r, t2, conv3(2), bn, relu=True, shortcut=t)
        with pytest.raises(ValueError):
            EF.conv_bn_act(r, t4, conv3(4), bn, relu=True, shortcut=EF.phase_split(r, t, 4))
        # non-divisible maps: refused by name before anything is launched
        del dilated_backend.calls[:]
        odd = r.input(torch.randn(1, 8, 6, 9))
        with pytest.raises(NotImplementedError, match=r'h = 6, w = 9.*d = 2'):
            EF.phase_split(r, odd, 2)
        with pytest.raises(NotImplementedError, match=r'h = 6, w = 9.*d = 4'):
            EF.phase_split(r, odd, 4)
        with pytest.raises(NotImplementedError):
            EF.phase_split(r, odd, 3)
        assert 'phase_split' not in dilated_backend.calls


def test_split_and_merge_nodes_are_each_others_backward(dilated_backend):
    """one tape node per call; the backward of a split is tok_phase_merge into the input's gradient (= first, += after)"""
    x = torch.randn(1, 8, 4, 4).to(BF).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    with engine.region() as r:
        t = r.input(x)
        n0 = len(r.nodes)
        a = EF.phase_split(r, t, 2)
        b = EF.phase_split(r, t, 2)
        assert len(r.nodes) == n0 + 2 and t.uses == 2
        oa, ob = r.output(EF.phase_merge(r, a, 2), EF.phase_merge(r, b, 2))
        assert len(r.nodes) == n0 + 4
    assert torch.equal(oa, x) and torch.equal(ob, x)
    del dilated_backend.calls[:]
    ga, gb = torch.randn(1, 8, 4, 4).to(BF), torch.randn(1, 8, 4, 4).to(BF)
    torch.autograd.backward([oa, ob], [ga, gb])
    assert dilated_backend.calls == ['phase_split', 'phase_split', 'phase_merge', 'phase_merge']   # the tape, backwards
    assert torch.equal(x.grad, (ga.float() + gb.float()).to(BF))


# ---- training ----------------------------------------------------------------------------------------------------------------
# 64 px, B = 2: resnet18 at output stride 8 splits inside its BasicBlocks (8 x 8 -> phase 2 -> phase 4); resnet26 runs its last
# Bottlenecks at phase 4 on 2 x 2 phase images; resnext50_32x4d at output stride 16 takes the grouped route at phase 2
@pytest.mark.parametrize('backbone,output_stride', [('resnet18', 8), ('resnet26', 8), ('resnext50_32x4d', 16)])
def test_training_step_vs_restatement(dev, backbone, output_stride):
    torch.manual_seed(0)
    task, ref = _pair(backbone, output_stride, dev)
    x, y = torch.randn(2, 3, 64, 64), torch.randint(0, 10, (2,))
    ref2 = copy.deepcopy(ref)
    ac_loss = _autocast_loss(ref2, x, y)
    ac_loss.backward()
    yard = {n: p.grad for n, p in ref2.named_parameters()}
    out = task.training_step({'image': x.to(dev), 'target': y.to(dev)}, 0)
    out['loss'].backward()
    ref_loss, _ = R.training_step(ref, {'image': x, 'target': y}, None)
    got, want, ac = float(out['loss'].detach()), float(ref_loss), float(ac_loss.detach())
    print(f'loss {got:.6f} fp32 {want:.6f} autocast {ac:.6f}')
    test = f'test_dilated_resnet::training_step[{dev}-{backbone}-os{output_stride}]'
    record_distance(test, 'loss', hip_vs_fp32=abs(got - want), autocast_vs_fp32=abs(ac - want))
    assert abs(got - want) < 1.5 * abs(ac - want) + 1e-2
    rp = dict(ref.named_parameters())
    for n, p in task.named_parameters():
        assert p.grad is not None, n
        mine, yardstick = rel_err(p.grad, rp[n].grad), rel_err(yard[n], rp[n].grad)
        record_distance(test, n, hip_vs_fp32=mine, autocast_vs_fp32=yardstick)
        assert mine < 1.5 * yardstick + 1e-2, n


@pytest.mark.parametrize('backbone,output_stride,lr', [('resnet18', 8, 0.002), ('resnet26', 8, 0.002),
                                                       ('resnext50_32x4d', 16, 0.0005)])
def test_two_optimizer_steps_read_the_updated_weights(dev, backbone, output_stride, lr):
    """The second step's loss comes from weights the optimizer has just changed: a stale copy of a weight would leave it at the
    first step's.  The rate is the one of tests/test_resnext.py (0.002, where that file explains it) except for the ResNeXt: at
    B = 2 one step at 0.002 takes its loss from 3.4 to 1.1, and in that regime the update amplifies the bf16 noise of the first
    step's gradients past what ONE autocast run measures — at the default output stride, which this feature does not touch,
    three seeds gave |mine - fp32| = 0.11, 0.48, 0.52 against |autocast - fp32| = 0.13, 0.26, 0.36.  At 0.0005 the step still
    moves the loss by 1.7 ... 1.9 (many times the yardstick) and autocast's own second-step distance stays at 0.015 ... 0.06."""
    torch.manual_seed(1)
    opt_params = {'lr': lr, 'momentum': 0.9, 'weight_decay': 1e-4}
    task, ref = _pair(backbone, output_stride, dev, opt_params=opt_params)
    ref2 = copy.deepcopy(ref)
    opt = task.configure_optimizers()[0]['optimizer']
    ropt, ropt2 = (torch.optim.SGD(m.parameters(), **opt_params) for m in (ref, ref2))
    x, y = torch.randn(2, 3, 64, 64), torch.randint(0, 10, (2,))
    losses = []
    for step in range(2):
        opt.zero_grad()
        out = task.training_step({'image': x.to(dev), 'target': y.to(dev)}, step)
        out['loss'].backward()
        opt.step()
        ref_loss, _ = R.training_step(ref, {'image': x, 'target': y}, ropt)
        ropt2.zero_grad(set_to_none=True)
        ac_loss = _autocast_loss(ref2, x, y)
        ac_loss.backward()
        ropt2.step()
        losses.append((float(out['loss'].detach()), float(ref_loss), float(ac_loss.detach())))
    print(losses)
    (g0, w0, _), (g1, w1, a1) = losses
    record_distance(f'test_dilated_resnet::second_step[{dev}-{backbone}-os{output_stride}]', 'loss', hip_vs_fp32=abs(g1 - w1),
                    autocast_vs_fp32=abs(a1 - w1))
    bound = 1.5 * abs(a1 - w1) + 1e-2
    assert abs(w1 - w0) > 10 * bound, 'the step must move the loss for the check to mean anything'
    assert abs(g1 - w1) < bound
    assert abs(g1 - w1) < 0.5 * abs(g0 - w1)          # nearer the updated model's loss than the first step's own


def test_forward_features_shapes_and_values(dev):
    torch.manual_seed(2)
    task, ref = _pair('resnet26', 8, dev)
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        feats = task.backbone.forward_features(x.to(dev))
        want = ref.backbone.forward_features(x)
        with torch.autocast('cpu', dtype=torch.bfloat16):
            ac = ref.backbone.forward_features(x)
    assert [tuple(f.shape) for f in feats] == [(2, 3, 64, 64), (2, 64, 32, 32), (2, 256, 16, 16), (2, 512, 8, 8),
                                               (2, 1024, 8, 8), (2, 2048, 8, 8)] == [tuple(f.shape) for f in want]
    for i in range(1, 6):
        mine, yardstick = rel_err(feats[i].float(), want[i]), rel_err(ac[i].float(), want[i])
        record_distance(f'test_dilated_resnet::forward_features[{dev}]', f'feature{i}', hip_vs_fp32=mine, autocast_vs_fp32=yardstick)
        assert mine < 1.5 * yardstick + 1e-2, i


def test_forward_features_train_every_consumer(dev):
    """in grad mode a dilated stage's map has two consumers (its merge and the next stage): a loss on every feature reaches
    every parameter, inside the yardstick"""
    torch.manual_seed(6)
    task, ref = _pair('resnet18', 8, dev)
    x = torch.randn(2, 3, 64, 64)
    loss_of = lambda fs: sum(f.float().square().mean() for f in fs[1:])      # noqa: E731
    loss_of(task.backbone.forward_features(x.to(dev))).backward()
    ref2 = copy.deepcopy(ref)
    with torch.autocast('cpu', dtype=torch.bfloat16):
        ac = loss_of(ref2.backbone.forward_features(x))
    ac.backward()
    loss_of(ref.backbone.forward_features(x)).backward()
    rp, yard = dict(ref.backbone.named_parameters()), dict(ref2.backbone.named_parameters())
    for n, p in task.backbone.named_parameters():
        assert p.grad is not None, n
        assert rel_err(p.grad, rp[n].grad) < 1.5 * rel_err(yard[n].grad, rp[n].grad) + 1e-2, n


@pytest.mark.parametrize('backbone,output_stride', [('resnet18', 8), ('resnext50_32x4d', 16)])
def test_eval_forward(dev, backbone, output_stride):
    torch.manual_seed(2)
    task, ref = _pair(backbone, output_stride, dev)
    task.eval()
    ref.eval()
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        got = task.forward(x.to(dev)).float().cpu()
        want = ref.forward_with_gt({'image': x, 'target': None})['prediction']
        with torch.autocast('cpu', dtype=torch.bfloat16):
            ac = ref.forward_with_gt({'image': x, 'target': None})['prediction'].float()
    assert got.shape == want.shape == (2, 10)
    mine, yardstick = rel_err(got, want), rel_err(ac, want)
    record_distance(f'test_dilated_resnet::eval_forward[{dev}-{backbone}]', 'prediction', hip_vs_fp32=mine, autocast_vs_fp32=yardstick)
    assert mine < 1.5 * yardstick + 1e-2


def test_no_grad_records_no_node(dilated_backend):
    m = T.BACKBONES.get('resnet18')(pretrained=False, output_stride=8).eval()
    seen = []
    real = engine.Region.add

    def spy(self, node):
        seen.append(type(node).__name__)
        return real(self, node)
    engine.Region.add = spy
    try:
        with torch.no_grad():
            m(torch.randn(2, 3, 64, 64))
        # layer3.0: block input + conv1 output; layer4.0: the same; forward() merges the last map alone: by 2, twice
        assert seen == [] and dilated_backend.calls.count('phase_split') == 4 and dilated_backend.calls.count('phase_merge') == 2
        del dilated_backend.calls[:]
        with torch.no_grad():
            m.forward_features(torch.randn(2, 3, 64, 64))
        assert seen == [] and dilated_backend.calls.count('phase_merge') == 3       # layer3's map by 2, layer4's by 2 twice
    finally:
        engine.Region.add = real


def test_frozen_dilated_weights_skip_the_weight_gradient(dev):
    torch.manual_seed(3)
    task, _ = _pair('resnet26', 8, dev)
    frozen = [n for n, p in task.named_parameters() if n.endswith('conv2.weight') and ('layer3' in n or 'layer4' in n)]
    assert len(frozen) == 4
    x, y = torch.randn(2, 3, 64, 64).to(dev), torch.randint(0, 10, (2,)).to(dev)
    runs = []
    for freeze in (False, True):
        for n, p in task.named_parameters():
            p.grad = None
            p.requires_grad_(not (freeze and n in frozen))
        out = task.training_step({'image': x, 'target': y}, 0)
        out['loss'].backward()
        runs.append({n: None if p.grad is None else p.grad.detach().clone() for n, p in task.named_parameters()})
    for n, g in runs[1].items():
        if n in frozen:
            assert g is None and runs[0][n] is not None, n
        else:
            assert g is not None and torch.equal(g, runs[0][n]), n


def test_output_stride_32_is_the_default_bit_for_bit(dev):
    torch.manual_seed(7)
    x, y = torch.randn(2, 3, 64, 64).to(dev), torch.randint(0, 10, (2,)).to(dev)
    runs = []
    for params in ({}, {'output_stride': 32}):
        cfg = cls_config('resnet26', 10, backbone_params=dict({'zero_init_last': False}, **params))
        task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
        task.load_state_dict(deterministic_state(task.state_dict(), 11))
        task.to(dev).train()
        out = task.training_step({'image': x, 'target': y}, 0)
        out['loss'].backward()
        runs.append((out['loss'].detach().clone(), {n: p.grad.clone() for n, p in task.named_parameters()},
                     [(n, _triple(m)) for n, m in task.named_modules() if isinstance(m, torch.nn.Conv2d)]))
    assert runs[0][2] == runs[1][2]
    assert torch.equal(runs[0][0], runs[1][0])
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(dilated_backend):
    m = T.BACKBONES.get('resnet18')(pretrained=False, output_stride=8)
    del dilated_backend.calls[:]
    with pytest.raises(NotImplementedError, match=r'h = 9, w = 9.*d = 2'):      # 72 px: the stride-8 map is 9 x 9
        m(torch.randn(1, 3, 72, 72))
    assert 'phase_split' not in dilated_backend.calls
    with pytest.raises(NotImplementedError):
        T.BACKBONES.get('resnet50d')(pretrained=False, output_stride=16)          # avg_down: no AvgPool2dSame
    with pytest.raises(NotImplementedError):
        T.BACKBONES.get('ecaresnet26t')(pretrained=False, output_stride=16)       # ECA's per-image mean is not phase-agnostic
    with pytest.raises(ValueError):
        T.BACKBONES.get('resnet50')(pretrained=False, output_stride=4)
    T.BACKBONES.get('resnet50d')(pretrained=False, output_stride=32)              # (both stay built at the default stride)
    T.BACKBONES.get('ecaresnet26t')(pretrained=False, output_stride=32)


# ---- GPU only ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_identical_steps_are_bit_identical():
    torch.manual_seed(4)
    task, _ = _pair('resnet26', 8, 'cuda')
    x, y = torch.randn(2, 3, 64, 64).cuda(), torch.randint(0, 10, (2,)).cuda()
    grads = []
    for _ in range(2):
        for p in task.parameters():
            p.grad = None
        out = task.training_step({'image': x, 'target': y}, 0)
        out['loss'].backward()
        torch.cuda.synchronize()
        grads.append((out['loss'].detach().clone(), {n: p.grad.clone() for n, p in task.named_parameters()}))
    assert torch.equal(grads[0][0], grads[1][0])
    for n in grads[0][1]:
        assert torch.equal(grads[0][1][n], grads[1][1][n]), n


@pytest.mark.gpu
def test_recipe_fit_on_device():
    from torchok_amd.run import fit
    cfg = T.load_config(os.path.join(RECIPES, 'classification_resnet18_os8.yaml'), overrides={'trainer.devices': 1})
    assert cfg.task.params.backbone_name == 'resnet18' and cfg.task.params.backbone_params.output_stride == 8
    g = torch.Generator().manual_seed(0)
    batches = [{'image': torch.randn(2, 3, 64, 64, generator=g).cuda(), 'target': torch.randint(0, 10, (2,), generator=g).cuda()}
               for _ in range(2)]
    seen = []
    res = fit(cfg, batches=batches, max_steps=2, device='cuda:0', on_step=lambda i, out: seen.append(float(out['loss'])))
    assert res['steps'] == 2 and len(seen) == 2 and all(v == v and abs(v) != float('inf') for v in seen)
    assert res['task'].backbone.layer4[1].conv2.dilation == (4, 4)
