"""Stochastic depth (drop_path_rate) in the ResNets, on the row-scaled BatchNorm unit (engine.functional.conv_bn_act(row_scale=...),
csrc/bn_droppath.hip).  Host side: the host-memory stand-in of the library plus tok_bn_droppath_* written here in torch over the
layouts the kernels use.  The per-block rates against the reference rule, the unchanged parameter tree, a training step of a basic
and a bottleneck network with PINNED draws inside the bf16 yardstick of the fp32 restatement (tests/resnet_droppath_ref.py) on
both routes of the other units, a dilated network, the gradient a DROPPED sample still sends through the batch statistics, eval
mode and rate 0 bit for bit and launch for launch the network without the argument, no_grad in train mode, the refusals, the
distribution of the draws, and on the GPU two identical steps bit for bit and the YAML recipe through the fit loop."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

import fake_backend as fb
import oracle.torchok_ref as R
import resnet_droppath_ref as P
import torchok_amd as T
from helpers import cls_config, copy_state, deterministic_state, record_distance, rel_err
from test_dilated_resnet import DilatedFake
from torchok_amd import engine
from torchok_amd.engine import functional as EF
from torchok_amd.models.backbones import resnet as resnet_mod
from torchok_amd.models.backbones.swin import DropPath

BF, F32 = torch.bfloat16, torch.float32
RECIPES = os.path.join(os.path.dirname(__file__), 'recipes')


class DropPathFake(DilatedFake):
    """FakeTok (+ tok_gconv_*, tok_phase_*) plus the tok_bn_droppath_* trio; records the y operand of every row-scaled unit
    and every `bn_y` a data-gradient epilogue is handed."""

    def __init__(self):
        super().__init__()
        self.drop_ys, self.rider_ys = [], []

    @staticmethod
    def _s(row_scale, rps, m):
        return fb._t(row_scale, (m // rps,), F32).repeat_interleave(rps).view(m, 1)

    def tok_bn_droppath_fwd(self, y, scale, shift, shortcut, row_scale, rps, out, mask, m, c, st):
        self.calls.append('bn_droppath_fwd')
        self.drop_ys.append(int(y))
        if m % rps or row_scale is None or shortcut is None:
            return -1
        z = fb._t(y, (m, c), BF).float() * fb._t(scale, (c,), F32) + fb._t(shift, (c,), F32)
        o = (self._s(row_scale, rps, m) * z + fb._t(shortcut, (m, c), BF).float()).clamp_min(0).to(BF)
        fb._t(out, (m, c), BF).copy_(o)
        if mask is not None:
            bits = (o.float() > 0).long().reshape(m, c // 8, 8)
            fb._t(mask, (m, c // 8), torch.uint8).copy_((bits << torch.arange(8)).sum(-1).to(torch.uint8))
        return 0

    def tok_bn_droppath_bwd_reduce(self, dout, y, mask, row_scale, rps, mean, rstd, m, c, partial, st):
        self.calls.append('bn_droppath_bwd_reduce')
        if m % rps or row_scale is None or mask is None:
            return -1
        dz = self._s(row_scale, rps, m) * (fb._t(dout, (m, c), BF).float() * self._bits(mask, m, c))
        xhat = (fb._t(y, (m, c), BF).float() - fb._t(mean, (c,), F32)) * fb._t(rstd, (c,), F32)
        p = fb._t(partial, (2, 1, c), F32)
        p[0, 0] = dz.sum(0)
        p[1, 0] = (dz * xhat).sum(0)
        return 0

    def tok_bn_droppath_bwd_apply(self, dout, y, mask, row_scale, rps, coef, dy, dshortcut, ds_acc, m, c, st):
        self.calls.append('bn_droppath_bwd_apply')
        if m % rps or row_scale is None or mask is None:
            return -1
        dt = fb._t(dout, (m, c), BF).float() * self._bits(mask, m, c)          # (read before dshortcut, which may alias dout, is written)
        co = fb._t(coef, (3, c), F32)
        res = co[0] * (self._s(row_scale, rps, m) * dt) + co[1] * fb._t(y, (m, c), BF).float() + co[2]
        fb._t(dy, (m, c), BF).copy_(res.to(BF))
        if dshortcut is not None:
            d = fb._t(dshortcut, (m, c), BF)
            d.copy_(((dt + d.float()) if ds_acc else dt).to(BF))
        return 0

    # every entry point whose epilogue can take over a producer's BatchNorm-backward sums
    def tok_conv_dgrad_bnstats(self, d, dy, wd, dx, accumulate, bn_y, bn_mask, partial, st):
        self.rider_ys.append(int(bn_y))
        return super().tok_conv_dgrad_bnstats(d, dy, wd, dx, accumulate, bn_y, bn_mask, partial, st)

    def tok_conv_dgrad_bias(self, d, dy, wd, bias, dx, accumulate, bn_y, bn_mask, partial, st):
        if bn_y is not None:
            self.rider_ys.append(int(bn_y))
        return super().tok_conv_dgrad_bias(d, dy, wd, bias, dx, accumulate, bn_y, bn_mask, partial, st)

    def tok_conv_dgrad_subacc(self, d, dy, wd, dx, dsub, bn_y, mask, partial, mask_store, st):
        if bn_y is not None:
            self.rider_ys.append(int(bn_y))
        return super().tok_conv_dgrad_subacc(d, dy, wd, dx, dsub, bn_y, mask, partial, mask_store, st)


@pytest.fixture
def drop_backend():
    token = fb.install(fake=DropPathFake())
    yield token[0]
    fb.uninstall(token)


@pytest.fixture(params=['host', pytest.param('hip', marks=pytest.mark.gpu)])
def dev(request):
    if request.param == 'host':
        request.getfixturevalue('drop_backend')
        return 'cpu'
    assert torch.cuda.is_available()
    return 'cuda'


@pytest.fixture
def pinned_draws(monkeypatch):
    """ResNet._run draws all of a step's vectors at once; with that switched off the vectors a test pins stay"""
    monkeypatch.setattr(resnet_mod, 'draw_drop_scales', lambda *a, **k: None)


def _pair(backbone, dev, rate, output_stride=32, seed=31):
    """the task on `dev` and the fp32 restatement with the same deterministic state, both in train mode"""
    params = {'zero_init_last': False, 'drop_path_rate': rate}
    if output_stride != 32:
        params['output_stride'] = output_stride
    cfg = cls_config(backbone, 10, backbone_params=params, inputs_shape=(3, 64, 64))
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
    ref = R.ClassificationModel(P.key(backbone, output_stride), 10, zero_init_last=False, drop_path_rate=rate)
    ref.load_state_dict(deterministic_state(ref.state_dict(), seed))
    copy_state(ref, task)
    task.to(dev).train()
    ref.train()
    return task, ref


def _autocast_loss(model, x, y):
    with torch.autocast('cpu', dtype=torch.bfloat16):
        o = model.forward_with_gt({'image': x, 'target': y})
    return F.cross_entropy(o['prediction'].float(), y)


def _rates(backbone):
    return [b.drop_path.drop_prob if b.drop_path is not None else 0.0 for b in P.blocks_of(backbone)]


# ---- construction ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,layers', [('resnet18', [2, 2, 2, 2]), ('resnet50', [3, 4, 6, 3]), ('resnext50_32x4d', [3, 4, 6, 3])])
def test_per_block_rates_and_parameter_tree(drop_backend, name, layers):
    plain = T.BACKBONES.get(name)(pretrained=False)
    mine = T.BACKBONES.get(name)(pretrained=False, drop_path_rate=0.2)
    want = P.block_rates(layers, 0.2)
    assert _rates(mine) == want and want[0] == 0.0 and want[-1] == 0.2
    blocks = P.blocks_of(mine)
    assert blocks[0].drop_path is None and all(isinstance(b.drop_path, DropPath) for b in blocks[1:])
    assert all(b.drop_path is None for b in P.blocks_of(plain))
    assert [(k, tuple(v.shape)) for k, v in mine.state_dict().items()] == [(k, tuple(v.shape)) for k, v in plain.state_dict().items()]
    ref = R.BACKBONES[P.key(name)](drop_path_rate=0.2)
    assert _rates(ref) == want
    assert [(k, tuple(v.shape)) for k, v in ref.state_dict().items()] == [(k, tuple(v.shape)) for k, v in mine.state_dict().items()]


@pytest.mark.parametrize('name,kw', [('resnet26t', {}), ('resnet50d', {}), ('wide_resnet50_2', {}), ('resnet34', {'output_stride': 8}),
                                     ('resnext101_32x8d', {'output_stride': 16})])
def test_other_entry_points_take_the_argument(drop_backend, name, kw):
    m = T.BACKBONES.get(name)(pretrained=False, drop_path_rate=0.1, **kw)
    rates = _rates(m)
    assert rates[0] == 0.0 and rates[-1] == 0.1 and rates == sorted(rates)


def test_refusals(drop_backend):
    from torchok_amd.models.backbones.resnet import BasicBlock, Bottleneck
    with pytest.raises(NotImplementedError, match='drop_block_rate'):
        T.BACKBONES.get('resnet50')(pretrained=False, drop_block_rate=0.1)
    with pytest.raises(NotImplementedError, match='eca'):
        T.BACKBONES.get('ecaresnet26t')(pretrained=False, drop_path_rate=0.1)
    for block in (BasicBlock, Bottleneck):
        with pytest.raises(NotImplementedError, match='eca'):
            block(64, 64, attn_layer='eca', drop_path=DropPath(0.1))
        # what was refused before stays refused, in the same words
        with pytest.raises(NotImplementedError, match=r"\['aa_layer'\] not built"):
            block(64, 64, aa_layer=torch.nn.AvgPool2d)
        with pytest.raises(NotImplementedError, match=r"\['attn_layer'\] not built"):
            block(64, 64, attn_layer='se')
        with pytest.raises(NotImplementedError, match=r"\['drop_block'\] not built"):
            block(64, 64, drop_block=object())
    T.BACKBONES.get('ecaresnet26t')(pretrained=False, drop_path_rate=0.0)         # rate 0 builds what it always built


def test_engine_refuses_what_the_unit_does_not_serve(drop_backend):
    from torchok_amd.models.backbones.resnet import BasicBlock
    blk = BasicBlock(16, 16).to(memory_format=torch.channels_last).train()
    s = torch.ones(2)
    with engine.region() as r:
        t = r.input(torch.randn(2, 16, 6, 6), c_pad_to=8)
        for kw in (dict(pool=True), dict(defer_apply=True), dict(act='relu6')):
            with pytest.raises(NotImplementedError, match='row_scale'):
                EF.conv_bn_act(r, t, blk.conv2, blk.bn2, relu=True, shortcut=t, row_scale=s, **kw)
        for kw in (dict(relu=False, shortcut=t), dict(relu=True), dict(relu=True, shortcut=t, bn=None)):
            with pytest.raises(ValueError, match='row_scale'):
                EF.conv_bn_act(r, t, blk.conv2, kw.pop('bn', blk.bn2), row_scale=s, **kw)
        for bad in (torch.ones(3), torch.ones(2, dtype=torch.float64), torch.ones(2, 1)):
            with pytest.raises(ValueError, match='one per sample'):
                EF.conv_bn_act(r, t, blk.conv2, blk.bn2, relu=True, shortcut=t, row_scale=bad)
    assert not any(c.startswith('bn_droppath') for c in drop_backend.calls)


# ---- training ----------------------------------------------------------------------------------------------------------------
# 64 px, B = 4, drop_path_rate 0.5: block k of the 8 has rate k / 14.  The draws are pinned: block 1 keeps every sample, the last
# block drops sample 1, the others as a seeded uniform draw says.
def _step_vs_restatement(dev, backbone, fused, monkeypatch, request, output_stride=32, test='training_step'):
    monkeypatch.setattr(EF, 'UNIT3_MIN_ROWS', 0 if fused else 1 << 40)
    torch.manual_seed(12)
    task, ref = _pair(backbone, dev, 0.5, output_stride)
    rates = _rates(ref.backbone)
    assert rates == _rates(task.backbone) == P.block_rates([2, 2, 2, 2], 0.5)
    scales = P.pinned_scales(rates, 4, seed=5, drop=((7, 1),), keep_all=(1,))
    assert float(scales[7][1]) == 0.0 and bool((scales[1] > 0).all()) and scales[0] is None
    x, y = torch.randn(4, 3, 64, 64), torch.randint(0, 10, (4,))
    ref2 = copy.deepcopy(ref)
    for model in (ref, ref2):
        P.pin(P.blocks_of(model.backbone), scales)
    ac_loss = _autocast_loss(ref2, x, y)
    ac_loss.backward()
    yard = {n: p.grad for n, p in ref2.named_parameters()}
    calls0 = None
    if dev == 'cpu':
        # the same step at rate 0 first: what the other units launch when no block has a rate
        fake = request.getfixturevalue('drop_backend')
        task0, _ = _pair(backbone, dev, 0.0, output_stride)
        task0.training_step({'image': x, 'target': y}, 0)['loss'].backward()
        calls0 = list(fake.calls)
        del fake.calls[:], fake.drop_ys[:], fake.rider_ys[:]
    P.pin(P.blocks_of(task.backbone), scales, dev)
    out = task.training_step({'image': x.to(dev), 'target': y.to(dev)}, 0)
    out['loss'].backward()
    ref_loss, _ = R.training_step(ref, {'image': x, 'target': y}, None)
    got, want, ac = float(out['loss'].detach()), float(ref_loss), float(ac_loss.detach())
    tag = f'test_resnet_droppath::{test}[{dev}-{backbone}-os{output_stride}-{"fused" if fused else "plain"}]'
    record_distance(tag, 'loss', hip_vs_fp32=abs(got - want), autocast_vs_fp32=abs(ac - want))
    print(f'loss {got:.6f} fp32 {want:.6f} autocast {ac:.6f}')
    rp = dict(ref.named_parameters())
    worst = []
    for n, p in task.named_parameters():
        assert p.grad is not None, n
        mine, yardstick = rel_err(p.grad, rp[n].grad), rel_err(yard[n], rp[n].grad)
        record_distance(tag, n, hip_vs_fp32=mine, autocast_vs_fp32=yardstick)
        print(f'{n}: {mine:.4e} (autocast {yardstick:.4e})')
        if not mine < 1.5 * yardstick + 1e-2:
            worst.append((n, mine, yardstick))
    assert abs(got - want) < 1.5 * abs(ac - want) + 1e-2
    assert not worst, worst
    if dev == 'cpu':
        calls = fake.calls
        for name in ('bn_droppath_fwd', 'bn_droppath_bwd_reduce', 'bn_droppath_bwd_apply'):
            assert calls.count(name) == 7, (name, calls.count(name))           # one trio per block with a rate
        # the seven units left the fused residual unit (a bottleneck's conv3 where it is taken at all) and nothing else moved
        lost = 7 if (fused and backbone == 'resnet26') else 0
        assert calls0.count('conv_fwd_bn_apply') - calls.count('conv_fwd_bn_apply') == lost
        assert (calls0.count('conv_fwd_bn_apply') > 0) == (fused and backbone == 'resnet26')
        assert len(fake.drop_ys) == len(set(fake.drop_ys)) == 7
        assert not set(fake.drop_ys) & set(fake.rider_ys), 'a data-gradient epilogue was handed the y of a row-scaled unit'
        assert len(fake.rider_ys) > 0                                          # (the other units still hand theirs over)


@pytest.mark.parametrize('backbone,fused', [('resnet18', True), ('resnet18', False), ('resnet26', True), ('resnet26', False)])
def test_training_step_vs_restatement(dev, backbone, fused, pinned_draws, monkeypatch, request):
    _step_vs_restatement(dev, backbone, fused, monkeypatch, request)


def test_dilated_network(dev, pinned_draws, monkeypatch, request):
    """output_stride 8: the row-scaled units of layers 3 and 4 run on phase images, rows_per_sample = h * w of the merged map"""
    _step_vs_restatement(dev, 'resnet18', False, monkeypatch, request, output_stride=8, test='dilated')


def test_dropped_sample_still_feeds_the_batch_statistics(dev, pinned_draws):
    """Sample 1 is dropped in the last block and every other draw keeps.  Changing that sample's image moves the gradient of the
    block's last convolution all the same: through the batch statistics of bn2 and through dy = c2 y + c3 on the sample's own
    rows.  The movement is the restatement's, by the yardstick, and a kernel that skipped dropped samples would show none of the
    second part."""
    torch.manual_seed(13)
    task, ref = _pair('resnet18', dev, 0.5)
    ref2 = copy.deepcopy(ref)
    rates = _rates(ref.backbone)
    scales = P.pinned_scales(rates, 4, seed=0, drop=((7, 1),), keep_all=range(7))
    x, y = torch.randn(4, 3, 64, 64), torch.randint(0, 10, (4,))
    x2 = x.clone()
    x2[1] = 2.0 * torch.randn(3, 64, 64)
    name = 'backbone.layer4.1.conv2.weight'
    grads = {}
    for which, img in (('a', x), ('b', x2)):
        for model in (ref, ref2):
            P.pin(P.blocks_of(model.backbone), scales)
            model.zero_grad(set_to_none=True)
        _autocast_loss(ref2, img, y).backward()
        R.training_step(ref, {'image': img, 'target': y}, None)
        for p in task.parameters():
            p.grad = None
        P.pin(P.blocks_of(task.backbone), scales, dev)
        task.training_step({'image': img.to(dev), 'target': y.to(dev)}, 0)['loss'].backward()
        grads[which] = [dict(m.named_parameters())[name].grad.detach().float().cpu().clone() for m in (task, ref, ref2)]
    mine, want, ac = (grads['b'][i] - grads['a'][i] for i in range(3))
    assert float(want.norm()) > 0.05 * float(grads['a'][1].norm()), 'the case must move the gradient for the check to mean anything'
    e, yardstick = rel_err(mine, want), rel_err(ac, want)
    record_distance(f'test_resnet_droppath::dropped_sample[{dev}]', name + ' (movement)', hip_vs_fp32=e, autocast_vs_fp32=yardstick)
    print(f'movement of {name}: {e:.4e} (autocast {yardstick:.4e}), |movement| / |gradient| {float(want.norm() / grads["a"][1].norm()):.3f}')
    assert e < 1.5 * yardstick + 1e-2


# ---- eval mode and rate 0: the network of today ----------------------------------------------------------------------------------
def _state_twin(backbone, dev, seed=17, **params):
    cfg = cls_config(backbone, 10, backbone_params=dict({'zero_init_last': False}, **params), inputs_shape=(3, 64, 64))
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
    task.load_state_dict(deterministic_state(task.state_dict(), seed))
    return task.to(dev)


@pytest.mark.parametrize('backbone', ['resnet18', 'resnet26'])
def test_rate_zero_and_eval_are_the_network_without_the_argument(dev, backbone, request):
    torch.manual_seed(8)
    x, y = torch.randn(2, 3, 64, 64).to(dev), torch.randint(0, 10, (2,)).to(dev)
    fake = request.getfixturevalue('drop_backend') if dev == 'cpu' else None
    train, evals = [], []
    for params in ({}, {'drop_path_rate': 0.0}, {'drop_path_rate': 0.3}):
        task = _state_twin(backbone, dev, **params)
        task.eval()                                                    # (first: a training step moves the running statistics)
        if fake:
            del fake.calls[:]
        with torch.no_grad():
            evals.append((task.forward(x).clone(), list(fake.calls) if fake else None))
        if params.get('drop_path_rate', 0.0) == 0.0:                   # train mode: rate 0 only
            task.train()
            if fake:
                del fake.calls[:]
            out = task.training_step({'image': x, 'target': y}, 0)
            out['loss'].backward()
            train.append((out['loss'].detach().clone(), {n: p.grad.clone() for n, p in task.named_parameters()},
                          list(fake.calls) if fake else None))
    assert torch.equal(train[0][0], train[1][0]) and train[0][2] == train[1][2]
    for n in train[0][1]:
        assert torch.equal(train[0][1][n], train[1][1][n]), n
    for out, calls in evals[1:]:
        assert torch.equal(out, evals[0][0]) and calls == evals[0][1]
    if fake:
        assert not any(c.startswith('bn_droppath') for c in train[0][2] + evals[2][1])


def test_no_grad_in_train_mode_drops_without_a_node(drop_backend, pinned_draws):
    m = T.BACKBONES.get('resnet18')(pretrained=False, drop_path_rate=0.5, zero_init_last=False).train()
    x = torch.randn(4, 3, 64, 64)
    scales = P.pinned_scales(_rates(m), 4, seed=5, drop=((7, 1),))
    seen = []
    real = engine.Region.add

    def spy(self, node):
        seen.append(type(node).__name__)
        return real(self, node)
    engine.Region.add = spy
    try:
        with torch.no_grad():
            P.pin(P.blocks_of(m), scales, 'cpu')
            dropped = m(x).float()
            P.pin(P.blocks_of(m), [None if s is None else torch.ones(4) for s in scales], 'cpu')
            kept = m(x).float()
    finally:
        engine.Region.add = real
    assert seen == [] and drop_backend.calls.count('bn_droppath_fwd') == 14
    assert not any(c.startswith('bn_droppath_bwd') for c in drop_backend.calls)
    assert not torch.equal(dropped, kept)
    assert all(b.drop_path is None or b.drop_path._drawn is None for b in P.blocks_of(m))      # every vector was consumed


def test_one_draw_per_step_reaches_every_block(drop_backend):
    """un-pinned: ResNet._run draws all vectors of the step at once, and each block consumes its own"""
    torch.manual_seed(3)
    m = T.BACKBONES.get('resnet18')(pretrained=False, drop_path_rate=0.5).train()
    seen = []
    real = DropPath.sample_scale

    def spy(self, batch, device):
        pre = getattr(self, '_drawn', None)
        s = real(self, batch, device)
        seen.append((pre is not None and s is pre, s.clone()))
        return s
    DropPath.sample_scale = spy
    try:
        m(torch.randn(4, 3, 64, 64))
    finally:
        DropPath.sample_scale = real
    assert len(seen) == 7 and all(drawn for drawn, _ in seen)
    for (_, s), rate in zip(seen, P.block_rates([2, 2, 2, 2], 0.5)[1:]):
        assert s.shape == (4,) and bool(((s == 0) | ((s - 1 / (1 - rate)).abs() < 1e-6)).all())


def test_distribution_of_the_draws():
    """2000 un-pinned draws of one DropPath(0.3) at B = 64: the kept fraction lies within 4 standard errors of 0.7, and a kept
    sample is scaled by 1 / 0.7"""
    torch.manual_seed(0)
    dp = DropPath(0.3).train()
    kept = total = 0
    for _ in range(2000):
        s = dp.sample_scale(64, torch.device('cpu'))
        assert bool(((s == 0) | ((s - 1 / 0.7).abs() < 1e-6)).all())
        kept += int((s > 0).sum())
        total += 64
    se = (0.7 * 0.3 / total) ** 0.5
    assert abs(kept / total - 0.7) < 4 * se, (kept / total, se)


# ---- GPU only ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_identical_steps_are_bit_identical(pinned_draws):
    torch.manual_seed(4)
    task, _ = _pair('resnet26', 'cuda', 0.5)
    scales = P.pinned_scales(_rates(task.backbone), 4, seed=5, drop=((7, 1),), keep_all=(1,))
    x, y = torch.randn(4, 3, 64, 64).cuda(), torch.randint(0, 10, (4,)).cuda()
    grads = []
    for _ in range(2):
        for p in task.parameters():
            p.grad = None
        P.pin(P.blocks_of(task.backbone), scales, 'cuda')
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
    cfg = T.load_config(os.path.join(RECIPES, 'classification_resnet50_droppath.yaml'), overrides={'trainer.devices': 1})
    assert cfg.task.params.backbone_name == 'resnet50' and cfg.task.params.backbone_params.drop_path_rate == 0.1
    g = torch.Generator().manual_seed(0)
    batches = [{'image': torch.randn(4, 3, 64, 64, generator=g).cuda(), 'target': torch.randint(0, 10, (4,), generator=g).cuda()}
               for _ in range(2)]
    seen = []
    res = fit(cfg, batches=batches, max_steps=2, device='cuda:0', on_step=lambda i, out: seen.append(float(out['loss'])))
    assert res['steps'] == 2 and len(seen) == 2 and all(v == v and abs(v) != float('inf') for v in seen)
    rates = _rates(res['task'].backbone)
    assert rates[0] == 0.0 and abs(rates[-1] - 0.1) < 1e-12 and len(rates) == 16
