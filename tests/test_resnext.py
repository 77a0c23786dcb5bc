"""The ResNeXt entry points of the reference (resnet.py:787-993) on the grouped 3x3 unit (engine.functional.gconv_bn_act,
csrc/conv_group.hip).  Host side: the host-memory stand-in of the library plus tok_gconv_* written here with torch's own grouped
convolution, over the layouts the kernels use.  Registered names, parameter trees against the plain-torch restatement
(tests/resnext_ref.py), a training step and two optimizer steps inside the bf16 yardstick of the fp32 restatement, eval
forward, feature shapes, frozen grouped weights, and on the GPU two identical steps bit for bit."""
import copy

import pytest
import torch
import torch.nn.functional as F

import fake_backend as fb
import oracle.torchok_ref as R
import resnext_ref as X
import torchok_amd as T
from helpers import cls_config, copy_state, deterministic_state, rel_err

BF, F32 = torch.bfloat16, torch.float32


class ResNeXtFake(fb.FakeTok):
    """FakeTok plus tok_gconv_*."""

    @staticmethod
    def _nchw(ptr, n, h, w, ld, c):
        return fb._t(ptr, (n, h, w, ld), BF)[..., :c].float().permute(0, 3, 1, 2)

    @staticmethod
    def _store(ptr, n, h, w, ld, c, val, accumulate):
        o = fb._t(ptr, (n, h, w, ld), BF)
        v = val.permute(0, 2, 3, 1)
        o[..., :c] = (v + o[..., :c].float() if accumulate else v).to(BF)
        return o[..., :c].float()

    @staticmethod
    def _weight(ptr, c, cg, krsc):
        """the (c, cg, 3, 3) view of the master (or its gradient slot) in the layout `krsc` names"""
        return fb._t(ptr, (c, 3, 3, cg), F32).permute(0, 3, 1, 2) if krsc else fb._t(ptr, (c, cg, 3, 3), F32)

    def tok_gconv_rows(self, n, h, wd, c, groups, stride):
        return 1

    def tok_gconv_fwd(self, x, w, krsc, n, h, wd, c, ld, groups, stride, out, stats, st):
        self.calls.append('gconv_fwd')
        wv = self._weight(w, c, c // groups, krsc).to(BF).float()
        y = F.conv2d(self._nchw(x, n, h, wd, ld, c), wv, stride=stride, padding=1, groups=groups)
        o = self._store(out, n, y.shape[2], y.shape[3], ld, c, y, 0).reshape(-1, c)
        if stats is not None:
            s = fb._t(stats, (2, 1, c), F32)
            s[0, 0], s[1, 0] = o.sum(0), (o * o).sum(0)
        return 0

    def tok_gconv_dgrad(self, dout, w, krsc, n, h, wd, c, ld, groups, stride, dx, accumulate, st):
        self.calls.append('gconv_dgrad')
        p, q = (h - 1) // stride + 1, (wd - 1) // stride + 1
        wv = self._weight(w, c, c // groups, krsc).to(BF).float()
        g = torch.nn.grad.conv2d_input((n, c, h, wd), wv, self._nchw(dout, n, p, q, ld, c), stride=stride, padding=1,
                                       groups=groups)
        self._store(dx, n, h, wd, ld, c, g, accumulate)
        return 0

    def tok_gconv_wgrad_ws_bytes(self, n, h, wd, c, groups, stride):
        return 4

    def tok_gconv_wgrad(self, x, dout, n, h, wd, c, ld, groups, stride, dw, krsc, accumulate, ws, ws_bytes, st):
        self.calls.append('gconv_wgrad')
        p, q = (h - 1) // stride + 1, (wd - 1) // stride + 1
        cg = c // groups
        g = torch.nn.grad.conv2d_weight(self._nchw(x, n, h, wd, ld, c), (c, cg, 3, 3), self._nchw(dout, n, p, q, ld, c),
                                        stride=stride, padding=1, groups=groups)
        t = self._weight(dw, c, cg, krsc)
        t.copy_(g + t if accumulate else g)
        return 0


@pytest.fixture
def resnext_backend():
    token = fb.install(fake=ResNeXtFake())
    yield token[0]
    fb.uninstall(token)


@pytest.fixture(params=['host', pytest.param('hip', marks=pytest.mark.gpu)])
def dev(request):
    if request.param == 'host':
        request.getfixturevalue('resnext_backend')
        return 'cpu'
    assert torch.cuda.is_available()
    return 'cuda'


def _pair(backbone, dev, seed=23, **opt):
    """the task on `dev` and the fp32 restatement with the same deterministic state, both in train mode"""
    cfg = cls_config(backbone, 10, backbone_params={'zero_init_last': False}, **opt)
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
    ref = R.ClassificationModel(backbone, 10, zero_init_last=False)
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
def test_registered_names(resnext_backend):
    assert all(n in T.BACKBONES.entrypoints for n in X.NAMES), [n for n in X.NAMES if n not in T.BACKBONES.entrypoints]
    for n in X.NOT_BUILT:               # group widths beyond 64: no kernel, so no entry point (the registry's KeyError)
        assert n not in T.BACKBONES.entrypoints
        with pytest.raises(KeyError):
            T.BACKBONES.get(n)
    for n in X.DEFAULT_PRETRAINED:      # the reference default asks for a download (pretrained=True)
        with pytest.raises(RuntimeError):
            T.BACKBONES.get(n)()


@pytest.mark.parametrize('name', ['resnext50_32x4d', 'resnext50d_32x4d', 'resnext101_32x8d', 'resnext101_64x4d'])
def test_parameter_tree_equals_the_restatement(resnext_backend, name):
    mine = T.BACKBONES.get(name)(pretrained=False, in_channels=3)
    ref = R.BACKBONES[name]()
    assert {k: tuple(v.shape) for k, v in mine.state_dict().items()} == \
        {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert mine.out_channels == ref.out_channels == 2048
    card, bw = (64, 4) if '64x4d' in name else (32, int(name.split('x')[-1][:-1]))
    for i, layer in enumerate((mine.layer1, mine.layer2, mine.layer3, mine.layer4)):
        for blk in layer:
            assert blk.conv2.groups == card and blk.conv2.weight.shape == (card * bw * 2 ** i, bw * 2 ** i, 3, 3)


def test_twins_build_the_same_network(resnext_backend):
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}      # noqa: E731
    for twin, of in X.TWINS.items():
        assert shapes(T.BACKBONES.get(twin)(pretrained=False)) == shapes(T.BACKBONES.get(of)(pretrained=False)), twin


def test_refusals_stay(resnext_backend):
    from torchok_amd.models.backbones.resnet import BasicBlock, Bottleneck
    with pytest.raises(AssertionError):
        BasicBlock(64, 64, cardinality=32, base_width=4)
    with pytest.raises(NotImplementedError):
        Bottleneck(64, 64, cardinality=32, base_width=4, attn_layer='se')
    with pytest.raises(NotImplementedError):
        Bottleneck(64, 64, cardinality=32, base_width=4, aa_layer=torch.nn.AvgPool2d)


def test_unserved_group_width_is_refused_by_name(resnext_backend):
    """group width 12 has no kernel: the unit says what is served instead of falling back"""
    from torchok_amd import engine
    from torchok_amd.engine import functional as EF
    conv = torch.nn.Conv2d(24, 24, 3, padding=1, groups=2, bias=False)
    bn = torch.nn.BatchNorm2d(24)
    with engine.region() as r:
        t = r.input(torch.randn(1, 24, 4, 4), c_pad_to=8)
        with pytest.raises(NotImplementedError, match=r'\(4, 8, 16, 32, 64\)'):
            EF.conv_bn_act(r, t, conv, bn, relu=True)


# ---- training ----------------------------------------------------------------------------------------------------------------
# resnext50d_32x4d at 72 px: 18 -> 9 -> 5 -> 3 maps, so the stride-2 grouped 3x3 and the ceil-mode average pool meet odd sizes
@pytest.mark.parametrize('backbone,size', [('resnext50_32x4d', 64), ('resnext50d_32x4d', 72)])
def test_training_step_vs_restatement(dev, backbone, size):
    torch.manual_seed(0)
    task, ref = _pair(backbone, dev)
    x, y = torch.randn(8, 3, size, size), torch.randint(0, 10, (8,))
    ref2 = copy.deepcopy(ref)
    ac_loss = _autocast_loss(ref2, x, y)
    ac_loss.backward()
    yard = {n: p.grad for n, p in ref2.named_parameters()}
    out = task.training_step({'image': x.to(dev), 'target': y.to(dev)}, 0)
    out['loss'].backward()
    ref_loss, _ = R.training_step(ref, {'image': x, 'target': y}, None)
    got, want, ac = float(out['loss'].detach()), float(ref_loss), float(ac_loss.detach())
    print(f'loss {got:.6f} fp32 {want:.6f} autocast {ac:.6f}')
    assert abs(got - want) < 1.5 * abs(ac - want) + 1e-2
    rp = dict(ref.named_parameters())
    for n, p in task.named_parameters():
        assert p.grad is not None, n
        assert rel_err(p.grad, rp[n].grad) < 1.5 * rel_err(yard[n], rp[n].grad) + 1e-2, n


def test_two_optimizer_steps_read_the_updated_weights(dev):
    """the second step's loss is computed from weights the optimizer has just changed: a stale copy of a grouped weight would
    leave it at the first step's.  The learning rate is small enough that the update itself does not amplify the bf16 noise
    of the first step's gradients past what one autocast run measures (after one step the stem's weights are
    4 % away from the fp32 restatement's at 0.002 and 19 % at 0.01, on resnet50 just as on resnext50_32x4d), and large enough that the step moves the
    loss by many times the yardstick."""
    torch.manual_seed(1)
    opt_params = {'lr': 0.002, 'momentum': 0.9, 'weight_decay': 1e-4}
    task, ref = _pair('resnext50_32x4d', dev, opt_params=opt_params)
    ref2 = copy.deepcopy(ref)
    opt = task.configure_optimizers()[0]['optimizer']
    ropt, ropt2 = (torch.optim.SGD(m.parameters(), **opt_params) for m in (ref, ref2))
    x, y = torch.randn(8, 3, 64, 64), torch.randint(0, 10, (8,))
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
    bound = 1.5 * abs(a1 - w1) + 1e-2
    assert abs(w1 - w0) > 10 * bound, 'the step must move the loss for the check to mean anything'
    assert abs(g1 - w1) < bound
    assert abs(g1 - w1) < 0.5 * abs(g0 - w1)          # nearer the updated model's loss than the first step's own


def test_eval_forward(dev):
    torch.manual_seed(2)
    task, ref = _pair('resnext50_32x4d', dev)
    task.eval()
    ref.eval()
    x = torch.randn(4, 3, 64, 64)
    with torch.no_grad():
        got = task.forward(x.to(dev)).float().cpu()
        want = ref.forward_with_gt({'image': x, 'target': None})['prediction']
        with torch.autocast('cpu', dtype=torch.bfloat16):
            ac = ref.forward_with_gt({'image': x, 'target': None})['prediction'].float()
    assert got.shape == want.shape == (4, 10)
    assert rel_err(got, want) < 1.5 * rel_err(ac, want) + 1e-2


def test_forward_features_shapes(dev):
    m = T.BACKBONES.get('resnext50d_32x4d')(pretrained=False).to(dev).eval()
    with torch.no_grad():
        feats = m.forward_features(torch.randn(2, 3, 72, 72).to(dev))
    assert [tuple(f.shape) for f in feats] == [(2, 3, 72, 72), (2, 64, 36, 36), (2, 256, 18, 18), (2, 512, 9, 9),
                                               (2, 1024, 5, 5), (2, 2048, 3, 3)]


def test_frozen_grouped_weights_skip_the_weight_gradient(dev, request):
    torch.manual_seed(3)
    task, _ = _pair('resnext50_32x4d', dev)
    frozen = [n for n, p in task.named_parameters() if n.endswith('conv2.weight')]
    assert len(frozen) == 16
    for n, p in task.named_parameters():
        if n in frozen:
            p.requires_grad_(False)
    x, y = torch.randn(8, 3, 64, 64), torch.randint(0, 10, (8,))
    out = task.training_step({'image': x.to(dev), 'target': y.to(dev)}, 0)
    out['loss'].backward()
    for n, p in task.named_parameters():
        assert (p.grad is None) == (n in frozen), n
        assert p.grad is None or bool(torch.isfinite(p.grad).all()), n
    if dev == 'cpu':
        calls = request.getfixturevalue('resnext_backend').calls
        assert calls.count('gconv_fwd') == 16 and calls.count('gconv_dgrad') == 16 and 'gconv_wgrad' not in calls


@pytest.mark.gpu
def test_two_identical_steps_are_bit_identical():
    torch.manual_seed(4)
    task, _ = _pair('resnext50_32x4d', 'cuda')
    x, y = torch.randn(8, 3, 64, 64).cuda(), torch.randint(0, 10, (8,)).cuda()
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
