"""MobileNetV3 backbones (torchok_amd/models/backbones/mobilenetv3.py) on the host-memory stand-in of the library: the
hard-swish BatchNorm and gated squeeze-excite entry points are written here in torch, over the layouts the kernels use.
Construction, state_dict layout, feature maps, a training step against the plain-torch restatement
(tests/mobilenetv3_ref.py), eval mode, frozen stages, the refusals and the recipe."""
import copy
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import fake_backend as fb
import mobilenetv3_ref as M
import torchok_amd as T
from helpers import cls_config, copy_state, deterministic_state, rel_err
from test_mnasnet import MnasFake

RECIPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'recipes')
BF = torch.bfloat16
F32 = torch.float32
NAMES = sorted(M.NAMES)


class V3Fake(MnasFake):
    """MnasFake plus tok_bn_hswish_* and tok_se_gate_*.  `hswish_y` collects the y pointers of the hard-swish units: a consumer
    epilogue that is handed one of them as bn_y would be reducing a hard-swish unit's sums with the ReLU rule."""

    def __init__(self):
        super().__init__()
        self.hswish_y = set()
        self.epilogue_y = []

    @staticmethod
    def _z(y, scale, shift, m, c):
        return fb._t(y, (m, c), BF).float() * fb._t(scale, (c,), F32) + fb._t(shift, (c,), F32)

    @staticmethod
    def _d(z):
        return torch.where(z < -3, torch.zeros_like(z), torch.where(z <= 3, z / 3 + 0.5, torch.ones_like(z)))

    def tok_bn_hswish_fwd(self, y, scale, shift, out, m, c, st):
        self.calls.append('bn_hswish_fwd')
        self.hswish_y.add(int(y))
        fb._t(out, (m, c), BF).copy_(F.hardswish(self._z(y, scale, shift, m, c)).to(BF))
        return 0

    def tok_bn_hswish_bwd_reduce(self, dout, y, scale, shift, mean, rstd, m, c, partial, st):
        self.calls.append('bn_hswish_bwd_reduce')
        dz = fb._t(dout, (m, c), BF).float() * self._d(self._z(y, scale, shift, m, c))
        xhat = (fb._t(y, (m, c), BF).float() - fb._t(mean, (c,), F32)) * fb._t(rstd, (c,), F32)
        p = fb._t(partial, (2, 1, c), F32)
        p[0, 0], p[1, 0] = dz.sum(0), (dz * xhat).sum(0)
        return 0

    def tok_bn_hswish_bwd_apply(self, dout, y, scale, shift, coef, dy, m, c, st):
        self.calls.append('bn_hswish_bwd_apply')
        dz = fb._t(dout, (m, c), BF).float() * self._d(self._z(y, scale, shift, m, c))
        co = fb._t(coef, (3, c), F32)
        fb._t(dy, (m, c), BF).copy_((co[0] * dz + co[1] * fb._t(y, (m, c), BF).float() + co[2]).to(BF))
        return 0

    def tok_se_gate_fwd(self, x, n, hw, c, ld, rd, kind, w1, b1, w2, b2, mean, hid, gate, ws, st):
        rc = self.tok_se_fwd(x, n, hw, c, ld, rd, w1, b1, w2, b2, mean, hid, gate, ws, st)
        if kind:
            self.calls[-1] = 'se_hsig_fwd'
            a = fb._t(hid, (n, rd), F32) @ fb._t(w2, (c, rd), F32).t() + fb._t(b2, (c,), F32)
            fb._t(gate, (n, c), F32).copy_(F.hardsigmoid(a))
        return rc

    def tok_se_gate_bwd(self, dout, x, n, hw, c, ld, rd, kind, w1, w2, mean, hid, gate, dw1, db1, dw2, db2, pacc, dx, dx_acc, ws,
                        st):
        if not kind:
            return self.tok_se_bwd(dout, x, n, hw, c, ld, rd, w1, w2, mean, hid, gate, dw1, db1, dw2, db2, pacc, dx, dx_acc, ws, st)
        self.calls.append('se_hsig_bwd')
        g = fb._t(dout, (n, hw, ld), BF)[..., :c].float()
        xv = fb._t(x, (n, hw, ld), BF)[..., :c].float()
        s = fb._t(gate, (n, c), F32)
        h = fb._t(hid, (n, rd), F32)
        ds = (g * xv).sum(1) * ((s > 0) & (s < 1)) / 6
        dh = (ds @ fb._t(w2, (c, rd), F32)) * (h > 0)
        dm = dh @ fb._t(w1, (rd, c), F32)
        for bit, (ptr_, shape, val) in enumerate(((dw1, (rd, c), dh.t() @ fb._t(mean, (n, c), F32)), (db1, (rd,), dh.sum(0)),
                                                  (dw2, (c, rd), ds.t() @ h), (db2, (c,), ds.sum(0)))):
            if ptr_ is not None:
                t = fb._t(ptr_, shape, F32)
                t.copy_(val + t if (pacc >> bit) & 1 else val)
        if dx is not None:
            o = fb._t(dx, (n, hw, ld), BF)
            v = g * s[:, None, :] + dm[:, None, :] / hw
            o[..., :c] = (v + o[..., :c].float() if dx_acc else v).to(BF)
        return 0

    # the consumer epilogues that reduce a producer's BatchNorm-backward sums: remember whose y they were given
    def tok_conv_dgrad_bnstats(self, d, dy, wd, dx, accumulate, bn_y, bn_mask, partial, st):
        self.epilogue_y.append(bn_y)
        return super().tok_conv_dgrad_bnstats(d, dy, wd, dx, accumulate, bn_y, bn_mask, partial, st)

    def tok_conv_dgrad_subacc(self, d, dy, wd, dx, dsub, bn_y, mask, partial, mask_store, st):
        self.epilogue_y.append(bn_y)
        return super().tok_conv_dgrad_subacc(d, dy, wd, dx, dsub, bn_y, mask, partial, mask_store, st)

    def tok_conv_dgrad_bias(self, d, dy, wd, bias, dx, accumulate, bn_y, bn_mask, partial, st):
        self.epilogue_y.append(bn_y)
        return super().tok_conv_dgrad_bias(d, dy, wd, bias, dx, accumulate, bn_y, bn_mask, partial, st)


@pytest.fixture
def v3_backend():
    token = fb.install(V3Fake())
    yield token[0]
    fb.uninstall(token)


# ---- construction and layout -------------------------------------------------------------------------------------------
# (type, in, mid, out, k, stride, se reduced width or 0, activation); mid of a 'ds' / 'cn' block is its input / output width
_LARGE = [('ds', 16, 16, 16, 3, 1, 0, 're'), ('ir', 16, 64, 24, 3, 2, 0, 're'), ('ir', 24, 72, 24, 3, 1, 0, 're'),
          ('ir', 24, 72, 40, 5, 2, 24, 're'), ('ir', 40, 120, 40, 5, 1, 32, 're'), ('ir', 40, 120, 40, 5, 1, 32, 're'),
          ('ir', 40, 240, 80, 3, 2, 0, 'hs'), ('ir', 80, 200, 80, 3, 1, 0, 'hs'), ('ir', 80, 184, 80, 3, 1, 0, 'hs'),
          ('ir', 80, 184, 80, 3, 1, 0, 'hs'), ('ir', 80, 480, 112, 3, 1, 120, 'hs'), ('ir', 112, 672, 112, 3, 1, 168, 'hs'),
          ('ir', 112, 672, 160, 5, 2, 168, 'hs'), ('ir', 160, 960, 160, 5, 1, 240, 'hs'), ('ir', 160, 960, 160, 5, 1, 240, 'hs'),
          ('cn', 160, 960, 960, 1, 1, 0, 'hs')]
_SMALL = [('ds', 16, 16, 16, 3, 2, 8, 're'), ('ir', 16, 72, 24, 3, 2, 0, 're'), ('ir', 24, 88, 24, 3, 1, 0, 're'),
          ('ir', 24, 96, 40, 5, 2, 24, 'hs'), ('ir', 40, 240, 40, 5, 1, 64, 'hs'), ('ir', 40, 240, 40, 5, 1, 64, 'hs'),
          ('ir', 40, 120, 48, 5, 1, 32, 'hs'), ('ir', 48, 144, 48, 5, 1, 40, 'hs'), ('ir', 48, 288, 96, 5, 2, 72, 'hs'),
          ('ir', 96, 576, 96, 5, 1, 144, 'hs'), ('ir', 96, 576, 96, 5, 1, 144, 'hs'), ('cn', 96, 576, 576, 1, 1, 0, 'hs')]
_SMALL_050 = [('ds', 16, 16, 8, 3, 2, 8, 're'), ('ir', 8, 40, 16, 3, 2, 0, 're'), ('ir', 16, 56, 16, 3, 1, 0, 're'),
              ('ir', 16, 64, 24, 5, 2, 16, 'hs'), ('ir', 24, 144, 24, 5, 1, 40, 'hs'), ('ir', 24, 144, 24, 5, 1, 40, 'hs'),
              ('ir', 24, 72, 24, 5, 1, 24, 'hs'), ('ir', 24, 72, 24, 5, 1, 24, 'hs'), ('ir', 24, 144, 48, 5, 2, 40, 'hs'),
              ('ir', 48, 288, 48, 5, 1, 72, 'hs'), ('ir', 48, 288, 48, 5, 1, 72, 'hs'), ('cn', 48, 288, 288, 1, 1, 0, 'hs')]
TABLES = {  # name -> (stem, blocks, blocks per stage, features (module, channels))
    'mobilenetv3_large_100': (16, _LARGE, [1, 2, 3, 4, 2, 3, 1], [('blocks.0.0', 16), ('blocks.1.1', 24), ('blocks.2.2', 40),
                                                                  ('blocks.4.1', 112), ('blocks.6.0', 960)]),
    'mobilenetv3_small_100': (16, _SMALL, [1, 2, 3, 2, 3, 1], [('act1', 16), ('blocks.0.0', 16), ('blocks.1.1', 24),
                                                               ('blocks.3.1', 48), ('blocks.5.0', 576)]),
    'mobilenetv3_small_050': (16, _SMALL_050, [1, 2, 3, 2, 3, 1], [('act1', 16), ('blocks.0.0', 8), ('blocks.1.1', 16),
                                                                   ('blocks.3.1', 24), ('blocks.5.0', 288)]),
}


def _bn(prefix, c):
    return {f'{prefix}.weight': (c,), f'{prefix}.bias': (c,), f'{prefix}.running_mean': (c,), f'{prefix}.running_var': (c,),
            f'{prefix}.num_batches_tracked': ()}


def _expected_state(stem, blocks, per_stage):
    exp = {'conv_stem.weight': (stem, 3, 3, 3), **_bn('bn1', stem)}
    names = [f'blocks.{s}.{i}' for s, n in enumerate(per_stage) for i in range(n)]
    assert len(names) == len(blocks)
    for name, (bt, cin, mid, cout, k, s, rd, act) in zip(names, blocks):
        se = {f'{name}.se.conv_reduce.weight': (rd, mid, 1, 1), f'{name}.se.conv_reduce.bias': (rd,),
              f'{name}.se.conv_expand.weight': (mid, rd, 1, 1), f'{name}.se.conv_expand.bias': (mid,)} if rd else {}
        if bt == 'ds':
            exp.update({f'{name}.conv_dw.weight': (cin, 1, k, k), **_bn(f'{name}.bn1', cin), **se,
                        f'{name}.conv_pw.weight': (cout, cin, 1, 1), **_bn(f'{name}.bn2', cout)})
        elif bt == 'ir':
            exp.update({f'{name}.conv_pw.weight': (mid, cin, 1, 1), **_bn(f'{name}.bn1', mid),
                        f'{name}.conv_dw.weight': (mid, 1, k, k), **_bn(f'{name}.bn2', mid), **se,
                        f'{name}.conv_pwl.weight': (cout, mid, 1, 1), **_bn(f'{name}.bn3', cout)})
        else:
            exp.update({f'{name}.conv.weight': (cout, cin, k, k), **_bn(f'{name}.bn1', cout)})
    return exp, names


@pytest.mark.parametrize('name', NAMES)
def test_every_entry_point_constructs(name):
    m = T.BACKBONES.get(name)(pretrained=False, in_channels=3)
    small = 'small' in name
    mult = {'050': 0.5, '075': 0.75}.get(name.split('_')[2], 1.0)
    assert type(m).__name__ == 'MobileNetV3' and m.num_features == (1024 if small else 1280)
    assert m.out_channels == M.make_divisible((576 if small else 960) * mult) == m.blocks[-1][0].conv.out_channels
    assert len(m.out_encoder_channels) == 5
    assert not hasattr(m, 'conv_head')


@pytest.mark.parametrize('name', sorted(TABLES))
def test_state_dict_features_and_stages_match_the_table(name):
    stem, blocks, per_stage, feats = TABLES[name]
    m = T.BACKBONES.get(name)()
    exp, block_names = _expected_state(stem, blocks, per_stage)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == exp
    assert list(m.state_dict()) == list(M.MobileNetV3(name).state_dict())          # timm's key order
    mods = dict(m.named_modules())
    for bn_, (bt, cin, mid, cout, k, s, rd, act) in zip(block_names, blocks):
        blk = mods[bn_]
        assert blk.relu == (act == 're'), bn_
        assert blk.has_skip == (bt != 'cn' and s == 1 and cin == cout), bn_
        conv = blk.conv if bt == 'cn' else blk.conv_dw
        assert conv.stride == (s, s) and conv.padding == (k // 2, k // 2)
    assert [f['module'] for f in m.feature_info] == [f for f, _ in feats]
    assert m.out_encoder_channels == tuple(c for _, c in feats)
    assert list(m.get_stages(0)) == [m.conv_stem, m.bn1, m.act1]
    assert list(m.get_stages(2))[3:] == [m.blocks[0], m.blocks[1]]
    assert len(m.get_stages(len(per_stage))) == 3 + len(per_stage)


def test_goog_init_statistics():
    torch.manual_seed(0)
    m = T.BACKBONES.get('mobilenetv3_large_100')()
    w = m.blocks[5][1].conv_dw.weight            # fan_out = 5 * 5 * 960 / 960 groups
    assert abs(float(w.detach().std()) - (2.0 / 25) ** 0.5) < 0.02
    assert float(m.blocks[5][1].se.conv_reduce.bias.abs().sum()) == 0.0
    assert float(m.blocks[6][0].bn1.weight.min()) == 1.0 and float(m.blocks[6][0].bn1.bias.abs().sum()) == 0.0


def test_small_050_feature_shapes_are_the_reference_tests(v3_backend):
    m = T.BACKBONES.get('mobilenetv3_small_050')(pretrained=False, in_channels=3).eval()
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        feats = m.forward_features(x)
        out = m(x)
    assert [tuple(f.shape) for f in feats] == [(2, 3, 64, 64), (2, 16, 32, 32), (2, 8, 16, 16), (2, 16, 8, 8), (2, 24, 4, 4),
                                               (2, 288, 2, 2)]
    assert tuple(out.shape) == (2, 288, 2, 2)
    assert m.out_channels == 288 and m.num_features == 1024
    assert torch.equal(feats[-1], out)


def test_state_dict_round_trips_with_the_restatement(v3_backend):
    ref = M.MobileNetV3('mobilenetv3_small_075')
    ref.load_state_dict(deterministic_state(ref.state_dict(), 9))
    m = T.BACKBONES.get('mobilenetv3_small_075')()
    m.load_state_dict(ref.state_dict())                                  # strict
    back = M.MobileNetV3('mobilenetv3_small_075')
    back.load_state_dict(m.state_dict())
    assert all(torch.equal(v, back.state_dict()[k]) for k, v in ref.state_dict().items())
    m.eval()
    ref.eval()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        mine, want = m.forward_features(x), ref.forward_features(x)
    assert len(mine) == len(want) == 6
    for a, b in zip(mine[1:], want[1:]):
        assert rel_err(a.float(), b) < 5e-2


# ---- refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kwargs,exc', [({'drop_path_rate': 0.1}, NotImplementedError), ({'output_stride': 16}, NotImplementedError),
                                        ({'act_layer': nn.SiLU}, NotImplementedError), ({'act_layer': nn.ReLU}, NotImplementedError),
                                        ({'norm_layer': nn.GroupNorm}, NotImplementedError),
                                        ({'pad_type': 'same'}, NotImplementedError),
                                        ({'se_layer': nn.Identity}, NotImplementedError),
                                        ({'pretrained': True}, RuntimeError)])
def test_refusals(kwargs, exc):
    with pytest.raises(exc):
        T.BACKBONES.get('mobilenetv3_small_100')(**kwargs)


@pytest.mark.parametrize('name', ['mobilenetv3_rw', 'tf_mobilenetv3_large_100', 'fbnetv3_b', 'lcnet_100'])
def test_other_family_members_stay_unregistered(name):
    with pytest.raises(KeyError):
        T.BACKBONES.get(name)


def test_engine_refuses_what_the_hard_swish_path_does_not_serve(v3_backend):
    from torchok_amd import engine
    from torchok_amd.engine import functional as EF
    conv, bn = nn.Conv2d(8, 8, 1, bias=False), nn.BatchNorm2d(8)
    dw = nn.Conv2d(8, 8, 3, padding=1, groups=8, bias=False)
    se = nn.Module()
    se.conv_reduce, se.conv_expand = nn.Conv2d(8, 8, 1), nn.Conv2d(8, 8, 1)
    with engine.region() as r:
        t = r.input(torch.randn(2, 8, 4, 4))
        for kw in ({'shortcut': t}, {'pool': True, 'relu': True}, {'defer_apply': True}):
            with pytest.raises(NotImplementedError):
                EF.conv_bn_act(r, t, conv, bn, act='hard_swish', **kw)
        with pytest.raises(NotImplementedError):
            EF.conv_bn_act(r, t, conv, None, act='hard_swish')
        with pytest.raises(NotImplementedError):
            EF.conv_bn_act(r, t, conv, bn, act='silu')
        with pytest.raises(NotImplementedError):
            EF.dwconv_bn_act(r, t, dw, bn, act='silu')
        with pytest.raises(NotImplementedError):
            EF.squeeze_excite(r, t, se, gate='tanh')
        r.output(EF.conv_bn_act(r, t, conv, bn, act='hard_swish'))
    assert v3_backend.calls.count('bn_hswish_fwd') == 1 and 'bn_act_fwd' not in v3_backend.calls


# ---- a training step on the stand-in against the restatement --------------------------------------------------------------
def _task(name, classes=10):
    cfg = cls_config(name, classes)
    return T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)


_BACKWARD = ('bn_hswish_bwd_reduce', 'bn_hswish_bwd_apply', 'bn_bwd_apply', 'se_hsig_bwd', 'se_bwd', 'dwconv_wgrad', 'dwconv_dgrad',
             'conv_wgrad', 'conv_dgrad')


@pytest.mark.parametrize('name', ['mobilenetv3_small_100', 'mobilenetv3_large_075'])
def test_training_step_matches_the_restatement(v3_backend, name):
    import oracle.torchok_ref as R
    torch.manual_seed(0)
    task = _task(name)
    ref = M.Classifier(name, 10)
    ref.load_state_dict(deterministic_state(ref.state_dict(), 3))
    copy_state(ref, task)
    task.train()
    ref.train()
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(4, 3, 64, 64, generator=g), torch.randint(0, 10, (4,), generator=g)
    ref2 = copy.deepcopy(ref)
    with torch.autocast('cpu', dtype=torch.bfloat16):
        o = ref2.forward_with_gt({'image': x, 'target': y})
    F.cross_entropy(o['prediction'].float(), y).backward()
    out = task.training_step({'image': x, 'target': y}, 0)
    out['loss'].backward()
    ref_loss, _ = R.training_step(ref, {'image': x, 'target': y}, None)
    assert abs(float(out['loss']) - float(ref_loss)) < 2e-2 * max(1.0, abs(float(ref_loss)))
    # the yardstick and the factors of test_mnasnet.py::test_training_step_matches_the_restatement (M.grad_scale: what the
    # distances of the analytically zero gradients are relative to)
    rp, ap = dict(ref.named_parameters()), dict(ref2.named_parameters())
    assert {n for n, _ in task.named_parameters()} == set(rp)
    for n, p in task.named_parameters():
        scale = M.grad_scale(n, rp)
        mine, yard = M.dist(p.grad, rp[n].grad, scale), M.dist(ap[n].grad, rp[n].grad, scale)
        assert mine < (6.0 if '.se.conv_reduce.' in n else 1.5) * yard + 2e-2, (n, mine, yard)
    rb = dict(ref.named_buffers())
    for n, b in task.named_buffers():
        if n in rb and n.endswith('running_var'):
            assert rel_err(b, rb[n]) < 2e-2, n
    calls = v3_backend.calls
    n_hs = sum(1 for m in task.backbone.modules() if getattr(m, 'relu', None) is False
               for _ in range({'InvertedResidual': 2}.get(type(m).__name__, 1))) + 1          # + the stem
    assert calls.count('bn_hswish_fwd') == calls.count('bn_hswish_bwd_reduce') == calls.count('bn_hswish_bwd_apply') == n_hs
    n_se = sum(1 for m in task.backbone.modules() if type(m).__name__ == 'SqueezeExcite')
    assert calls.count('se_hsig_fwd') == calls.count('se_hsig_bwd') == n_se > 0
    assert 'se_fwd' not in calls and 'se_bwd' not in calls
    assert not any(c in calls for c in ('conv_fwd_bn_apply', 'bn_gram_finalize', 'bn3_bwd_prepare', 'relu_mask_reduce'))  # unit 3
    # the consumer epilogues served ReLU / linear producers only
    assert len(v3_backend.hswish_y) == n_hs
    assert not [p for p in v3_backend.epilogue_y if p is not None and int(p) in v3_backend.hswish_y]
    assert 'dgrad_bnstats' in calls             # ... and they still serve those (the ReLU blocks, the linear projections)


def test_eval_mode_and_no_grad_forward(v3_backend):
    task = _task('mobilenetv3_large_100')
    ref = M.Classifier('mobilenetv3_large_100', 10)
    ref.load_state_dict(deterministic_state(ref.state_dict(), 5))
    copy_state(ref, task)
    task.eval()
    ref.eval()
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        mine = task.backbone(x).float()
        want = ref.backbone(x)
        feats = task.backbone.forward_features(x)
    assert rel_err(mine, want) < 5e-2
    assert [tuple(f.shape[1:]) for f in feats[1:]] == [(16, 32, 32), (24, 16, 16), (40, 8, 8), (112, 4, 4), (960, 2, 2)]
    assert 'bn_hswish_fwd' in v3_backend.calls and 'se_hsig_fwd' in v3_backend.calls
    assert not [c for c in v3_backend.calls if c in _BACKWARD]
    # grad mode, eval-mode BatchNorm (frozen statistics): the backward runs on coef = (scale, 0, 0)
    for p in task.parameters():
        if p.dim() == 1:
            p.requires_grad_(False)              # BatchNorm affine gradients are not served in eval mode (nor biases here)
    del v3_backend.calls[:]
    x.requires_grad_(False)
    out = task.backbone(x)
    out.float().square().mean().backward()
    assert 'bn_hswish_bwd_apply' in v3_backend.calls and 'bn_hswish_bwd_reduce' not in v3_backend.calls
    assert task.backbone.conv_stem.weight.grad is not None


def test_frozen_stages_launch_nothing_for_the_frozen_blocks(v3_backend):
    task = _task('mobilenetv3_small_100')
    frozen = task.backbone.get_stages(3)                 # the stem and stages 0-2: the first hard-swish blocks included
    frozen_params = list(frozen.parameters())
    for p in frozen_params:
        p.requires_grad_(False)
    before = [p.detach().clone() for p in frozen_params]
    task.train()
    opt = task.configure_optimizers()[0]['optimizer']
    g = torch.Generator().manual_seed(1)
    out = task.training_step({'image': torch.randn(4, 3, 64, 64, generator=g), 'target': torch.randint(0, 10, (4,), generator=g)}, 0)
    out['loss'].backward()
    opt.step()
    assert all(p.grad is None for p in frozen_params)
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, frozen_params))
    calls = v3_backend.calls
    n_dw = sum(1 for m in task.backbone.modules() if isinstance(m, nn.Conv2d) and m.groups > 1)
    n_dw_frozen = sum(1 for m in frozen.modules() if isinstance(m, nn.Conv2d) and m.groups > 1)
    n_se = sum(1 for m in task.backbone.modules() if type(m).__name__ == 'SqueezeExcite')
    n_se_frozen = sum(1 for m in frozen.modules() if type(m).__name__ == 'SqueezeExcite')
    assert n_dw_frozen == 6 and n_se_frozen == 4
    assert calls.count('dwconv_wgrad') == calls.count('dwconv_dgrad') == n_dw - n_dw_frozen
    assert calls.count('se_hsig_bwd') == n_se - n_se_frozen and calls.count('se_hsig_fwd') == n_se
    # stage 2's two hard-swish blocks and the stem are frozen: 2 x 3 + 1 units run forward only
    assert calls.count('bn_hswish_fwd') - calls.count('bn_hswish_bwd_apply') == 7
    live = [p for p in task.backbone.parameters() if p.requires_grad]
    assert live and all(p.grad is not None for p in live)


# ---- the recipe ----------------------------------------------------------------------------------------------------------
def test_recipe_drives_a_training_step(v3_backend):
    cfg = T.load_config(os.path.join(RECIPES, 'classification_mobilenetv3.yaml'))
    assert cfg.task.params.backbone_name == 'mobilenetv3_small_100'
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params).train()
    assert type(task.backbone).__name__ == 'MobileNetV3' and task.head.fc.in_features == 576
    opt = task.configure_optimizers()[0]['optimizer']
    assert type(opt).__name__ == 'SGD'
    torch.manual_seed(0)
    out = task.training_step({'image': torch.randn(4, 3, 64, 64), 'target': torch.randint(0, 10, (4,))}, 0)
    assert torch.isfinite(out['loss'])
    opt.zero_grad()
    out['loss'].backward()
    assert all(p.grad is not None for p in task.parameters())
    opt.step()
    task.on_train_epoch_end()
    assert any(k.startswith('train/') for k in task.logged)


def test_recipe_through_the_fit_loop(v3_backend):
    from torchok_amd.run import fit
    cfg = T.load_config(os.path.join(RECIPES, 'classification_mobilenetv3.yaml'), overrides={'trainer.devices': 1})
    torch.manual_seed(0)
    seen = []
    batches = [{'image': torch.randn(4, 3, 64, 64), 'target': torch.randint(0, 10, (4,))} for _ in range(2)]
    res = fit(cfg, batches=batches, max_steps=2, device='cpu', on_step=lambda i, out: seen.append(float(out['loss'])))
    assert res['steps'] == 2 and len(seen) == 2 and all(v == v for v in seen)
