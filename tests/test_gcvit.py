"""GCViT backbones (torchok_amd/models/backbones/gcvit.py) on the host-memory stand-in of the library: the window-attention
entry points with the shared query and the squeeze-excite entry points with the inner activation are written here in torch,
over the layouts the kernels use.  Registration, the refusals, the engine wiring of a small model against the plain-torch
restatement (tests/gcvit_ref.py), feature maps, eval / no-grad, state dicts both ways, the recipe, and what squeeze_excite gained."""
import copy
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import fake_backend as fb
import gcvit_ref as R
import torchok_amd as T
from helpers import cls_config, copy_state, rel_err
from test_beit import BeitFake
from test_mnasnet import MnasFake

RECIPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'recipes')
BF, F32 = torch.bfloat16, torch.float32
TINY_BP = {k: v for k, v in R.TINY.items()}            # what gcvit_xxtiny needs to be told to become the 64 px model


class GcFake(BeitFake, MnasFake):
    """BeitFake (relative-position bias, LayerScale) and MnasFake (squeeze-excite) plus tok_gc_attn_* and tok_se_act_*."""

    def _attn(self, qkv, ld, qg, ldg, bias, ldb, b, h, w, c, heads, ws):
        n, parts = ws * ws, 2 if qg is not None else 3
        x = fb._t(qkv, (b * h * w, ld), BF)[:, :parts * c].float().clone().requires_grad_(True)
        g = None if qg is None else fb._t(qg, (b * n, ldg), BF)[:, :c].float().clone().requires_grad_(True)
        bs = fb._t(bias, (heads, n, ldb), F32)[..., :n].clone().requires_grad_(True)
        q, k, v, idx = R._qkv(x, g, (b, h, w, heads, ws))
        s = (q @ k.transpose(-2, -1)) * R.SCALE + bs.unsqueeze(0)
        return x, g, bs, s, R._rows(s.softmax(-1) @ v, idx, b * h * w)

    def _refused(self, c, heads, h, w, ws, lse):
        if c != heads * 32 or h % ws or w % ws or ws * ws > 256 or lse is None:
            self._err = b'tok_gc_attn: geometry not served'
            return True
        return False

    def tok_gc_attn_fwd(self, qkv, ld, qg, ldg, bias, ldb, b, h, w, c, heads, ws, out, ldo, lse, st):
        self.calls.append('gc_attn_global_fwd' if qg is not None else 'gc_attn_local_fwd')
        if self._refused(c, heads, h, w, ws, lse):
            return -1
        assert ldb >= ws * ws and ldb % 4 == 0
        with torch.no_grad():
            _, _, _, s, o = self._attn(qkv, ld, qg, ldg, bias, ldb, b, h, w, c, heads, ws)
        fb._t(lse, tuple(s.shape[:3]), F32).copy_(torch.logsumexp(s, -1))
        fb._t(out, (b * h * w, ldo), BF)[:, :c] = o.to(BF)
        return 0

    def tok_gc_attn_bwd_ws_bytes(self, b, h, w, heads, ws, is_global, want_dbias):
        return 4 * b * h * w * heads + (4 * heads * ws ** 4 if want_dbias else 0)

    def tok_gc_attn_bwd(self, qkv, ld, qg, ldg, bias, ldb, out, dout, ldo, lse, b, h, w, c, heads, ws, dqkv, ldd, dqg, lddg, dbias,
                        dbias_acc, ws_buf, ws_bytes, st):
        self.calls.append('gc_attn_global_bwd' if qg is not None else 'gc_attn_local_bwd')
        if self._refused(c, heads, h, w, ws, lse):
            return -1
        n, parts = ws * ws, 2 if qg is not None else 3
        with torch.enable_grad():
            x, g, bs, _, o = self._attn(qkv, ld, qg, ldg, bias, ldb, b, h, w, c, heads, ws)
            grads = torch.autograd.grad(o, (x, bs) + ((g,) if g is not None else ()), fb._t(dout, (b * h * w, ldo), BF)[:, :c].float())
        fb._t(dqkv, (b * h * w, ldd), BF)[:, :parts * c] = grads[0].to(BF)
        if g is not None:
            fb._t(dqg, (b * n, lddg), BF)[:, :c] = grads[2].to(BF)
        if dbias is not None:
            self.calls.append('gc_attn_dbias')
            t = fb._t(dbias, (heads, n, ldb), F32)
            t[..., :n] = grads[1] + t[..., :n] if dbias_acc else grads[1]
        return 0

    def tok_se_act_ws_floats(self, n, hw, c, rd):
        return 1

    @staticmethod
    def _se(x, n, hw, c, ld, rd, w1, b1, w2, b2, act_kind):
        m = fb._t(x, (n, hw, ld), BF)[..., :c].float().mean(1)
        pre = m @ fb._t(w1, (rd, c), F32).t() + (0 if b1 is None else fb._t(b1, (rd,), F32))
        h = F.gelu(pre) if act_kind else F.relu(pre)
        return m, pre, h, h @ fb._t(w2, (c, rd), F32).t() + (0 if b2 is None else fb._t(b2, (c,), F32))

    def tok_se_act_fwd(self, x, n, hw, c, ld, rd, gate_kind, act_kind, w1, b1, w2, b2, mean, hid, gate, ws, st):
        self.calls.append('se_act_fwd:%s:%s' % ('gelu' if act_kind else 'relu', 'nobias' if b1 is None else 'bias'))
        assert (b1 is None) == (b2 is None) and gate_kind == 0
        m, pre, h, a = self._se(x, n, hw, c, ld, rd, w1, b1, w2, b2, act_kind)
        fb._t(mean, (n, c), F32).copy_(m)
        fb._t(hid, (n, rd), F32).copy_(pre if act_kind else h)        # GELU: the pre-activation is kept
        fb._t(gate, (n, c), F32).copy_(torch.sigmoid(a))
        return 0

    def tok_se_act_bwd(self, dout, x, n, hw, c, ld, rd, gate_kind, act_kind, w1, w2, mean, hid, gate, dw1, db1, dw2, db2, pacc, dx,
                       dx_acc, ws, st):
        self.calls.append('se_act_bwd')
        g = fb._t(dout, (n, hw, ld), BF)[..., :c].float()
        xv = fb._t(x, (n, hw, ld), BF)[..., :c].float()
        s = fb._t(gate, (n, c), F32)
        kept = fb._t(hid, (n, rd), F32)
        ds = (g * xv).sum(1) * s * (1 - s)
        if act_kind:
            pre = kept.clone().requires_grad_(True)
            with torch.enable_grad():
                h = F.gelu(pre)
                dact, = torch.autograd.grad(h.sum(), pre)
            h = h.detach()
        else:
            h, dact = kept, (kept > 0).float()
        dh = (ds @ fb._t(w2, (c, rd), F32)) * dact
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


@pytest.fixture
def gc_backend():
    token = fb.install(GcFake())
    yield token[0]
    fb.uninstall(token)


# ---- registration and layout -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(R.VARIANTS))
def test_every_entry_point_constructs_with_the_reference_parameter_count(name):
    with torch.device('meta'):
        m = T.BACKBONES.get(name)(pretrained=False, in_channels=3)
    e = R.VARIANTS[name].get('embed_dim', 64)
    assert type(m).__name__ == 'GlobalContextVit' and m.out_channels == 8 * e
    assert m.encoder_channels == [e, 2 * e, 4 * e, 8 * e] and m.out_encoder_channels == (e, 2 * e, 4 * e, 8 * e)
    assert [len(s.blocks) for s in m.stages] == list(R.VARIANTS[name]['depths'])
    assert [s.blocks[0].attn.num_heads for s in m.stages] == list(R.VARIANTS[name]['num_heads'])
    assert [s.window_size for s in m.stages] == [(7, 7), (7, 7), (14, 14), (7, 7)]
    assert [[b.attn.use_global for b in s.blocks][:2] for s in m.stages] == [[False, True]] * 4
    assert sum(p.numel() for p in m.parameters()) == R.BACKBONE_PARAMS[name]
    assert isinstance(m.stages[0].blocks[0].ls1, nn.Identity) == ('layer_scale' not in R.VARIANTS[name])


def test_missing_name_was_a_key_error_and_the_new_names_are_registered():
    for name in R.VARIANTS:
        assert callable(T.BACKBONES.get(name))


@pytest.mark.parametrize('name', ['gcvit_xxtiny', 'gcvit_small'])
def test_state_dict_interchanges_with_the_restatement(name):
    m = T.BACKBONES.get(name)(pretrained=False, **TINY_BP)
    ref = R.GlobalContextVit(**dict(R.VARIANTS[name], **R.TINY))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    R.ref_state(ref, 1)
    assert not any(m.load_state_dict(ref.state_dict(), strict=True))            # no missing, no unexpected keys
    ref2 = R.GlobalContextVit(**dict(R.VARIANTS[name], **R.TINY))
    ref2.load_state_dict(m.state_dict(), strict=True)
    for k, v in ref.state_dict().items():
        assert torch.equal(v, ref2.state_dict()[k]), k


def test_load_state_dict_can_leave_the_tables_alone():
    m = T.BACKBONES.get('gcvit_xxtiny')(load_relative_position_bias_table=False, **TINY_BP)
    ref = R.ref_state(R.GlobalContextVit(**dict(R.VARIANTS['gcvit_xxtiny'], **R.TINY)), 2)
    before = m.stages[0].blocks[0].attn.rel_pos.relative_position_bias_table.detach().clone()
    res = m.load_state_dict(ref.state_dict(), strict=False)
    assert all('relative_position_bias_table' in k for k in res.missing_keys) and len(res.missing_keys) == 8
    assert torch.equal(m.stages[0].blocks[0].attn.rel_pos.relative_position_bias_table.detach(), before)
    assert torch.equal(m.stem.conv1.weight.detach(), ref.stem.conv1.weight.detach())


def test_init_schemes_no_weight_decay_and_get_stages():
    torch.manual_seed(0)
    m = T.BACKBONES.get('gcvit_xxtiny')(**TINY_BP)
    fc = m.stages[2].blocks[0].mlp.fc1
    assert abs(float(fc.weight.detach().std()) - 0.02) < 2e-3 and float(fc.bias.detach().abs().sum()) == 0.0
    v = T.BACKBONES.get('gcvit_xxtiny')(weight_init='vit', **TINY_BP)
    fc = v.stages[2].blocks[0].mlp.fc1
    bound = (6.0 / (fc.in_features + fc.out_features)) ** 0.5
    assert float(fc.weight.detach().abs().max()) <= bound and float(fc.weight.detach().abs().max()) > 0.9 * bound
    assert 0 < float(fc.bias.detach().abs().max()) < 1e-4
    assert float(v.stages[2].blocks[0].attn.proj.bias.detach().abs().sum()) == 0.0
    nwd = m.no_weight_decay()
    assert len(nwd) == 8 and all(k.endswith('attn.rel_pos.relative_position_bias_table') for k in nwd)
    st = m.get_stages(2)
    assert len(st) == 3 and st[0] is m.stem and st[2] is m.stages[1]


# ---- refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kwargs,exc', [
    ({'drop_rate': 0.1}, NotImplementedError), ({'proj_drop_rate': 0.1}, NotImplementedError),
    ({'attn_drop_rate': 0.1}, NotImplementedError), ({'act_layer': 'relu'}, NotImplementedError),
    ({'norm_layer': 'batchnorm2d'}, NotImplementedError), ({'norm_layer_cl': 'rmsnorm'}, NotImplementedError),
    ({'embed_dim': 96}, NotImplementedError),                                   # 96 / 2 heads: head_dim 48
    ({'num_heads': (1, 4, 8, 16)}, NotImplementedError),
    ({'img_size': 200}, NotImplementedError),                                   # 50 x 50 tokens, windows of 6
    ({'img_size': 576}, NotImplementedError),                                   # windows of 18 x 18 = 324 tokens
    ({'window_size': ((7, 14), (7, 7), (14, 14), (7, 7))}, NotImplementedError),
    ({'pretrained': True}, RuntimeError)])
def test_refusals(kwargs, exc):
    with pytest.raises(exc), torch.device('meta'):
        T.BACKBONES.get('gcvit_xxtiny')(**dict(dict(depths=(1, 1, 1, 1)), **kwargs))


def test_engine_refuses_what_the_kernel_does_not_serve(gc_backend):
    from torchok_amd import engine
    from torchok_amd.engine import transformer as ET
    from torchok_amd.engine.core import TTensor
    with torch.no_grad(), engine.region() as r:
        qkv = TTensor(torch.zeros(2 * 8 * 8, 96, dtype=BF), 96)
        for geo in ((2, 8, 8, 32, 2, 4), (2, 8, 8, 32, 1, 3), (2, 8, 8, 32, 1, 17)):
            with pytest.raises(NotImplementedError):
                ET.gc_window_attention(r, qkv, geo, (torch.zeros(1, 16, 16), None))
    assert not gc_backend.calls


# ---- forward and training steps against the restatement ----------------------------------------------------------------------
def _task_and_ref(name='gcvit_xxtiny', seed=3, bp=None):
    cfg = cls_config(name, 10, backbone_params=dict(TINY_BP, **(bp or {})), inputs_shape=(3, 64, 64))
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
    ref = R.ref_state(R.Classifier(10, **dict(R.VARIANTS[name], **R.TINY)), seed)
    copy_state(ref, task)
    return task, ref


def test_forward_features_eval_and_no_grad(gc_backend):
    task, ref = _task_and_ref(seed=4)
    task.eval()
    ref.eval()
    x = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        feats = task.backbone.forward_features(x)
        want = ref.backbone.forward_features(x)
        y = task.backbone(x)
    assert [tuple(f.shape) for f in feats] == [(3, 3, 64, 64), (3, 32, 16, 16), (3, 64, 8, 8), (3, 128, 4, 4), (3, 256, 2, 2)]
    assert feats[0] is x
    for a, b in zip(feats[1:], want[1:]):
        assert rel_err(a.float(), b) < 3e-2
    assert rel_err(y.float(), want[-1]) < 3e-2 and not y.requires_grad
    calls = gc_backend.calls
    assert calls.count('gc_attn_local_fwd') == 8 and calls.count('gc_attn_global_fwd') == 8          # two forwards, 4 + 4 each
    assert 'se_act_fwd:gelu:nobias' in calls and 'se_fwd' not in calls
    assert not any(c.endswith('_bwd') for c in calls)


@pytest.mark.parametrize('name', ['gcvit_xxtiny', 'gcvit_small'])
def test_training_step_matches_the_restatement(gc_backend, name):
    torch.manual_seed(0)
    task, ref = _task_and_ref(name)
    task.train()
    ref.train()
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(3, 3, 64, 64, generator=g), torch.randint(0, 10, (3,), generator=g)      # B = 3, nW = 16 / 4 / 1 / 1
    ref2 = copy.deepcopy(ref)
    with torch.autocast('cpu', dtype=torch.bfloat16):
        o = ref2(x)
    F.cross_entropy(o.float(), y).backward()
    out = task.training_step({'image': x, 'target': y}, 0)
    out['loss'].backward()
    ref_loss = F.cross_entropy(ref(x), y)
    ref_loss.backward()
    assert abs(float(out['loss']) - float(ref_loss)) < 2e-2 * max(1.0, abs(float(ref_loss)))
    rp, ap = dict(ref.named_parameters()), dict(ref2.named_parameters())
    seen = set()
    for n, p in task.named_parameters():
        assert p.grad is not None, n
        mine, yard = rel_err(p.grad, rp[n].grad), rel_err(ap[n].grad, rp[n].grad)
        # the gates of tests/test_mnasnet.py: x1.5 + 2e-2, and x6 for the first squeeze-excite layer, whose gradient is the residual
        # of a cancelling sum over each image of d(out) * x times s (1 - s) formed from bf16-stored gradients (the stand-in
        # rounds where the kernels round; autocast keeps that path in fp32)
        assert mine < (6.0 if '.se.fc1.' in n else 1.5) * yard + 2e-2, (n, mine, yard)
        seen.add(n)
    assert seen == set(rp)
    calls = gc_backend.calls
    for what in ('gc_attn_local_bwd', 'gc_attn_global_bwd', 'gc_attn_dbias', 'relpos_bias_bwd', 'se_act_bwd'):
        assert what in calls, what
    assert calls.count('relpos_bias_fwd') == 16                  # gathered in the forward and again in the backward of 8 blocks
    assert ('layer_scale_dgamma' in calls) == (name == 'gcvit_small')


def test_stage_input_gradient_matches_the_restatement(gc_backend):
    """the image takes no gradient in this engine; the input of a stage does.  Stage 1: downsample, a global_block with one pool
    level, a local and a global block; its input feeds the first block and the global_block."""
    torch.manual_seed(0)
    ref = R.ref_state(R.GlobalContextVit(**dict(R.VARIANTS['gcvit_xxtiny'], **R.TINY)), 6).stages[1]
    m = T.BACKBONES.get('gcvit_xxtiny')(**TINY_BP).stages[1]
    m.load_state_dict(ref.state_dict())
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 32, 16, 16, generator=g).to(BF)
    dout = torch.randn(3, 64, 8, 8, generator=g).to(BF)
    xr = x.float().requires_grad_()
    ref(xr).backward(dout.float())
    xa = x.float().requires_grad_()
    ref2 = copy.deepcopy(ref)
    with torch.autocast('cpu', dtype=torch.bfloat16):
        ya = ref2(xa)
    ya.float().backward(dout.float())
    xe = x.contiguous(memory_format=torch.channels_last).requires_grad_()
    ye = m(xe)
    ye.backward(dout.contiguous(memory_format=torch.channels_last))
    assert rel_err(ye.float(), ref(x.float())) < 3e-2
    assert rel_err(xe.grad.float(), xr.grad) < 1.5 * rel_err(xa.grad, xr.grad) + 2e-2


def test_frozen_tables_take_no_gradient(gc_backend):
    task, _ = _task_and_ref()
    for n, p in task.named_parameters():
        if 'relative_position_bias_table' in n:
            p.requires_grad_(False)
    task.train()
    out = task.training_step({'image': torch.randn(2, 3, 64, 64), 'target': torch.randint(0, 10, (2,))}, 0)
    out['loss'].backward()
    assert all(p.grad is None for n, p in task.named_parameters() if 'relative_position_bias_table' in n)
    calls = gc_backend.calls
    assert 'gc_attn_global_bwd' in calls and 'gc_attn_dbias' not in calls and 'relpos_bias_bwd' not in calls


def test_drop_path_rates_reach_the_blocks(gc_backend):
    task, _ = _task_and_ref(bp=dict(drop_path_rate=0.7))
    blocks = [b for s in task.backbone.stages for b in s.blocks]
    assert type(blocks[0].drop_path1).__name__ == 'Identity'
    assert abs(blocks[-1].drop_path2.drop_prob - 0.7) < 1e-6 and abs(blocks[1].drop_path1.drop_prob - 0.1) < 1e-6
    task.train()
    out = task.training_step({'image': torch.randn(4, 3, 64, 64), 'target': torch.randint(0, 10, (4,))}, 0)
    out['loss'].backward()
    assert float(out['loss']) == float(out['loss'])


# ---- the recipe through the fit loop --------------------------------------------------------------------------------------------
def test_gcvit_recipe_through_the_fit_loop(gc_backend):
    from torchok_amd.run import fit
    os.environ.setdefault('HOME', '/root')
    shrink = {'task.params.backbone_params.' + k: (list(v) if isinstance(v, tuple) else v) for k, v in TINY_BP.items()}
    cfg = T.load_config(os.path.join(RECIPES, 'classification_gcvit_xxtiny.yaml'), overrides=dict({'trainer.devices': 1}, **shrink))
    assert cfg.task.params.backbone_name == 'gcvit_xxtiny' and cfg.optimization[0].optimizer.name == 'AdamW'
    torch.manual_seed(0)
    seen = []
    batches = [{'image': torch.randn(2, 3, 64, 64), 'target': torch.randint(0, 10, (2,))} for _ in range(2)]
    res = fit(cfg, batches=batches, max_steps=2, device='cpu', on_step=lambda i, out: seen.append(float(out['loss'])))
    assert res['steps'] == 2 and len(seen) == 2 and all(v == v for v in seen)
    assert 'gc_attn_global_bwd' in gc_backend.calls and 'se_act_bwd' in gc_backend.calls


# ---- what squeeze_excite gained ----------------------------------------------------------------------------------------------------
class _Se(nn.Module):
    def __init__(self, c, rd, bias, names):
        super().__init__()
        setattr(self, names[0], nn.Conv2d(c, rd, 1, bias=bias))
        setattr(self, names[1], nn.Conv2d(rd, c, 1, bias=bias))


@pytest.mark.parametrize('act,bias,names', [('gelu', False, ('fc1', 'fc2')), ('gelu', True, ('fc1', 'fc2')),
                                            ('relu', False, ('conv_reduce', 'conv_expand')),
                                            ('relu', True, ('conv_reduce', 'conv_expand'))])
def test_squeeze_excite_variants(gc_backend, act, bias, names):
    from torchok_amd import engine
    from torchok_amd.engine import functional as EF
    torch.manual_seed(0)
    c, rd = 16, 8
    se = _Se(c, rd, bias, names)
    x = torch.randn(2, c, 5, 5).to(BF)
    dout = torch.randn(2, c, 5, 5).to(BF)
    xe = x.contiguous(memory_format=torch.channels_last).requires_grad_()
    with engine.region() as r:
        kw = {} if (act, names) == ('relu', ('conv_reduce', 'conv_expand')) and bias else dict(act=act, names=names)
        y = r.output(EF.squeeze_excite(r, r.input(xe), se, **kw))
    y.backward(dout.contiguous(memory_format=torch.channels_last))
    fc1, fc2 = getattr(se, names[0]), getattr(se, names[1])
    prm = [fc1.weight.detach().view(rd, c), fc2.weight.detach().view(c, rd)] + \
        ([fc1.bias.detach(), fc2.bias.detach()] if bias else [None, None])
    out_r, _, dx_r, grads = R.se_ref(x.permute(0, 2, 3, 1).reshape(2, 25, c), *prm, act=act,
                                     dout=dout.permute(0, 2, 3, 1).reshape(2, 25, c))
    assert rel_err(y.float().permute(0, 2, 3, 1).reshape(2, 25, c), out_r) < 1e-2
    assert rel_err(xe.grad.float().permute(0, 2, 3, 1).reshape(2, 25, c), dx_r) < 2e-2
    assert rel_err(fc1.weight.grad.view(rd, c), grads[0]) < 1e-3 and rel_err(fc2.weight.grad.view(c, rd), grads[1]) < 1e-3
    if bias:
        assert rel_err(fc1.bias.grad, grads[2]) < 1e-3 and rel_err(fc2.bias.grad, grads[3]) < 1e-3
    calls = gc_backend.calls
    if act == 'relu' and bias:
        assert 'se_fwd' in calls and 'se_bwd' in calls and not any(k.startswith('se_act') for k in calls)     # the old launches
    else:
        assert 'se_act_fwd:%s:%s' % (act, 'bias' if bias else 'nobias') in calls and 'se_act_bwd' in calls and 'se_fwd' not in calls


def test_squeeze_excite_refuses_an_unknown_activation_and_one_sided_biases(gc_backend):
    from torchok_amd import engine
    from torchok_amd.engine import functional as EF
    se = _Se(16, 8, True, ('conv_reduce', 'conv_expand'))
    x = torch.randn(1, 16, 3, 3).to(BF).contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), engine.region() as r:
        t = r.input(x)
        with pytest.raises(NotImplementedError):
            EF.squeeze_excite(r, t, se, act='silu')
        se.conv_expand.bias = None
        with pytest.raises(NotImplementedError):
            EF.squeeze_excite(r, t, se)
