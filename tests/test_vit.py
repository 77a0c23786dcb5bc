"""Vision Transformer backbones (torchok_amd/models/backbones/vit.py) on the host-memory stand-in of the library: the new
global-attention, patch-gather, token-assembly and row-select entry points are written here in torch, over the same layouts
the kernels use.  Registration, state_dict layout, the reference's known output shapes, training steps against the plain-torch
restatement (tests/vit_ref.py), frozen stages with the get_stages holder quirk, the refusals and run.fit over a recipe."""
import copy
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import fake_backend as fb
import torchok_amd as T
import vit_ref as V
from helpers import copy_state, rel_err
from torchok_amd.constructor.config import apply_schema

RECIPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'recipes')
BF = torch.bfloat16
F32 = torch.float32

SERVED = {  # name -> (patch, embed_dim, depth, heads, img_size, qkv_bias, pre_norm)
    'vit_tiny_patch16_224': (16, 192, 12, 3, 224, True, False), 'vit_tiny_patch16_384': (16, 192, 12, 3, 384, True, False),
    'vit_small_patch32_224': (32, 384, 12, 6, 224, True, False), 'vit_small_patch32_384': (32, 384, 12, 6, 384, True, False),
    'vit_small_patch16_224': (16, 384, 12, 6, 224, True, False), 'vit_small_patch16_384': (16, 384, 12, 6, 384, True, False),
    'vit_base_patch32_224': (32, 768, 12, 12, 224, True, False), 'vit_base_patch32_384': (32, 768, 12, 12, 384, True, False),
    'vit_base_patch16_224': (16, 768, 12, 12, 224, True, False), 'vit_base_patch16_384': (16, 768, 12, 12, 384, True, False),
    'vit_base_patch8_224': (8, 768, 12, 12, 224, True, False),
    'vit_large_patch32_224': (32, 1024, 24, 16, 224, True, False), 'vit_large_patch32_384': (32, 1024, 24, 16, 384, True, False),
    'vit_large_patch16_224': (16, 1024, 24, 16, 224, True, False), 'vit_large_patch16_384': (16, 1024, 24, 16, 384, True, False),
    'vit_large_patch14_224': (14, 1024, 24, 16, 224, True, False),
    'vit_tiny_patch16_224_in21k': (16, 192, 12, 3, 224, True, False), 'vit_small_patch32_224_in21k': (32, 384, 12, 6, 224, True, False),
    'vit_small_patch16_224_in21k': (16, 384, 12, 6, 224, True, False), 'vit_base_patch32_224_in21k': (32, 768, 12, 12, 224, True, False),
    'vit_base_patch16_224_in21k': (16, 768, 12, 12, 224, True, False), 'vit_base_patch8_224_in21k': (8, 768, 12, 12, 224, True, False),
    'vit_large_patch32_224_in21k': (32, 1024, 24, 16, 224, True, False),
    'vit_large_patch16_224_in21k': (16, 1024, 24, 16, 224, True, False),
    'vit_base_patch16_224_sam': (16, 768, 12, 12, 224, True, False), 'vit_base_patch32_224_sam': (32, 768, 12, 12, 224, True, False),
    'vit_small_patch16_224_dino': (16, 384, 12, 6, 224, True, False), 'vit_small_patch8_224_dino': (8, 384, 12, 6, 224, True, False),
    'vit_base_patch16_224_dino': (16, 768, 12, 12, 224, True, False), 'vit_base_patch8_224_dino': (8, 768, 12, 12, 224, True, False),
    'vit_base_patch16_224_miil_in21k': (16, 768, 12, 12, 224, False, False),
    'vit_base_patch16_224_miil': (16, 768, 12, 12, 224, False, False),
    'vit_base_patch32_224_clip_laion2b': (32, 768, 12, 12, 224, True, True),
    'vit_large_patch14_224_clip_laion2b': (14, 1024, 24, 16, 224, True, True),
}
UNSERVED = ['vit_huge_patch14_224', 'vit_giant_patch14_224', 'vit_gigantic_patch14_224', 'vit_huge_patch14_224_in21k',
            'vit_base_patch32_plus_256', 'vit_base_patch16_plus_240', 'vit_small_patch16_36x1_224',
            'vit_small_patch16_18x2_224', 'vit_base_patch16_18x2_224', 'vit_base_patch16_rpn_224',
            'vit_huge_patch14_224_clip_laion2b', 'vit_giant_patch14_224_clip_laion2b']


class VitFake(fb.FakeTok):
    """FakeTok plus tok_global_attn_*, tok_patch_gather, tok_vit_embed_* and tok_rows_select."""

    @staticmethod
    def _qkv(qkv, ldq, b, n, heads):
        c = heads * 64
        x = fb._t(qkv, (b, n, ldq), BF)[..., :3 * c].float()
        return x.reshape(b, n, 3, heads, 64).permute(2, 0, 3, 1, 4)

    def tok_global_attn_fwd(self, qkv, ldq, b, n, heads, head_dim, out, ldo, lse, st):
        if head_dim != 64:
            self._err = b'tok_global_attn_fwd: head_dim not served'
            return -1
        self.calls.append('global_attn_fwd')
        q, k, v = self._qkv(qkv, ldq, b, n, heads)
        s = (q @ k.transpose(-2, -1)) * 0.125
        fb._t(lse, (b, heads, n), F32).copy_(torch.logsumexp(s, -1))
        o = (s.softmax(-1) @ v).transpose(1, 2).reshape(b, n, heads * 64)
        fb._t(out, (b, n, ldo), BF)[..., :heads * 64] = o.to(BF)
        return 0

    def tok_global_attn_bwd_ws_bytes(self, b, n, heads):
        return 4 * b * n * heads

    def tok_global_attn_bwd(self, qkv, ldq, out, dout, ldo, lse, b, n, heads, head_dim, dqkv, ldd, ws, ws_bytes, st):
        self.calls.append('global_attn_bwd')
        c = heads * 64
        x = fb._t(qkv, (b, n, ldq), BF)[..., :3 * c].float().clone().requires_grad_(True)
        with torch.enable_grad():
            q, k, v = x.reshape(b, n, 3, heads, 64).permute(2, 0, 3, 1, 4)
            o = (((q @ k.transpose(-2, -1)) * 0.125).softmax(-1) @ v).transpose(1, 2).reshape(b, n, c)
            g, = torch.autograd.grad(o, x, fb._t(dout, (b, n, ldo), BF)[..., :c].float())
        fb._t(dqkv, (b, n, ldd), BF)[..., :3 * c] = g.to(BF)
        return 0

    def tok_patch_gather(self, img, n, h, w, p, rows, st):
        self.calls.append('patch_gather')
        x = fb._t(img, (n, h // p, p, w // p, p, 4), BF)
        fb._t(rows, (n, h // p, w // p, p, p, 4), BF).copy_(x.permute(0, 1, 3, 2, 4, 5))
        return 0

    def tok_vit_embed_fwd(self, patch, pos, cls, b, n_p, d, no_embed_class, out, st):
        self.calls.append('vit_embed_fwd')
        x = fb._t(patch, (b, n_p, d), BF).float()
        prefix = 1 if cls is not None else 0
        ps = fb._t(pos, (n_p if no_embed_class else n_p + prefix, d), F32)
        if no_embed_class:
            x = x + ps
            if prefix:
                x = torch.cat((fb._t(cls, (1, 1, d), F32).expand(b, -1, -1), x), 1)
        else:
            if prefix:
                x = torch.cat((fb._t(cls, (1, 1, d), F32).expand(b, -1, -1), x), 1)
            x = x + ps
        fb._t(out, (b, n_p + prefix, d), BF).copy_(x.to(BF))
        return 0

    def tok_vit_embed_bwd(self, dout, b, n_p, d, has_cls, no_embed_class, dpos, pos_acc, dcls, cls_acc, st):
        self.calls.append('vit_embed_bwd')
        prefix = 1 if has_cls else 0
        g = fb._t(dout, (b, n_p + prefix, d), BF).float()
        if dpos is not None:
            self.calls.append('vit_embed_dpos')
            v = (g[:, prefix:] if no_embed_class else g).sum(0)
            t = fb._t(dpos, tuple(v.shape), F32)
            t.copy_(v + t if pos_acc else v)
        if dcls is not None:
            self.calls.append('vit_embed_dcls')
            v = g[:, 0].sum(0)
            t = fb._t(dcls, (d,), F32)
            t.copy_(v + t if cls_acc else v)
        return 0

    def tok_rows_select(self, src, b, t, first, count, d, dst, direction, accumulate, st):
        self.calls.append('rows_select')
        if direction == 0:
            fb._t(dst, (b, count, d), BF).copy_(fb._t(src, (b, t, d), BF)[:, first:first + count])
            return 0
        o = fb._t(dst, (b, t, d), BF)
        g = fb._t(src, (b, count, d), BF).float()
        if accumulate:
            o[:, first:first + count] = (o[:, first:first + count].float() + g).to(BF)
        else:
            o.zero_()
            o[:, first:first + count] = g.to(BF)
        return 0


@pytest.fixture
def vit_backend():
    token = fb.install(VitFake())
    yield token[0]
    fb.uninstall(token)


def vit_config(backbone, num_classes=10, optimizer='SGD', opt_params=None, backbone_params=None, side=32):
    """cls_config of tests/helpers.py without a pooling stage: the head reads the backbone's (B, D) output."""
    cfg = {
        'task': {'name': 'ClassificationTask',
                 'params': {'backbone_name': backbone,
                            'backbone_params': dict({'pretrained': False, 'in_channels': 3}, **(backbone_params or {})),
                            'head_name': 'ClassificationHead', 'head_params': {'num_classes': num_classes},
                            'inputs': [{'shape': [3, side, side], 'dtype': 'float32'}]}},
        'joint_loss': {'losses': [{'name': 'CrossEntropyLoss', 'mapping': {'input': 'prediction', 'target': 'target'}}]},
        'optimization': [{'optimizer': {'name': optimizer,
                                        'params': opt_params or {'lr': 0.1, 'momentum': 0.9, 'weight_decay': 1e-4}}}],
        'data': {}, 'trainer': {'precision': 'bf16'},
    }
    return apply_schema(cfg)


def vit_task(backbone='vit_tiny_patch16_224', **kw):
    cfg = vit_config(backbone, **kw)
    return T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)


def ref_state(ref, seed):
    """Every parameter non-trivial: LayerNorm affines off (1, 0), biases off 0, cls_token / pos_embed of unit-ish size."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if n.endswith('norm1.weight') or n.endswith('norm2.weight') or n.endswith('norm.weight') or 'norm_pre.weight' in n:
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1 or n in ('cls_token', 'pos_embed'):
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / p[0].numel()) ** 0.5)
    return ref


# ---- registration and layout -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(SERVED))
def test_every_served_entry_point_constructs(name):
    patch, dim, depth, heads, img, qkv_bias, pre_norm = SERVED[name]
    m = T.BACKBONES.get(name)(pretrained=False, in_channels=3, weight_init='skip')
    assert type(m).__name__ == 'VisionTransformer' and m.out_channels == dim and m.num_features == dim
    assert m.out_encoder_channels == (dim,) * 4
    assert m.patch_embed.img_size == (img, img) and m.patch_embed.patch_size == (patch, patch)
    assert len(m.blocks) == depth and m.blocks[0].attn.num_heads == heads
    assert (m.blocks[0].attn.qkv.bias is not None) == qkv_bias
    assert (m.patch_embed.proj.bias is None) == pre_norm
    assert isinstance(m.norm_pre, nn.LayerNorm) == pre_norm
    assert m.norm.eps == (1e-5 if pre_norm else 1e-6)
    assert tuple(m.pos_embed.shape) == (1, (img // patch) ** 2 + 1, dim)


@pytest.mark.parametrize('name', UNSERVED)
def test_unserved_entry_points_stay_unregistered(name):
    with pytest.raises(KeyError):
        T.BACKBONES.get(name)


@pytest.mark.parametrize('kwargs', [{}, dict(qkv_bias=False, pre_norm=True, norm_layer=nn.LayerNorm),
                                    dict(class_token=False), dict(no_embed_class=True)])
def test_state_dict_matches_the_restatement(kwargs):
    m = T.BACKBONES.get('vit_tiny_patch16_224')(img_size=32, depth=2, **kwargs)
    ref = V.VisionTransformer(img_size=32, patch_size=16, embed_dim=192, depth=2, num_heads=3, **kwargs)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert got == want
    assert list(m.state_dict()) == list(ref.state_dict())


def test_timm_state_dict_names():
    m = T.BACKBONES.get('vit_small_patch16_224')(depth=1)
    names = set(m.state_dict())
    for k in ('patch_embed.proj.weight', 'patch_embed.proj.bias', 'cls_token', 'pos_embed', 'blocks.0.norm1.weight',
              'blocks.0.attn.qkv.weight', 'blocks.0.attn.qkv.bias', 'blocks.0.attn.proj.weight', 'blocks.0.norm2.bias',
              'blocks.0.mlp.fc1.weight', 'blocks.0.mlp.fc2.bias', 'norm.weight', 'norm.bias'):
        assert k in names, k
    assert tuple(m.state_dict()['pos_embed'].shape) == (1, 197, 384)


def test_init_weights():
    torch.manual_seed(0)
    m = T.BACKBONES.get('vit_base_patch16_224')(depth=2)
    assert abs(float(m.blocks[0].attn.qkv.weight.detach().std()) - 0.02) < 2e-3
    assert float(m.blocks[1].mlp.fc2.bias.abs().sum()) == 0.0
    assert float(m.cls_token.abs().max()) < 1e-5 and float(m.cls_token.abs().max()) > 0
    assert abs(float(m.pos_embed.std()) - 0.02) < 2e-3
    assert float(m.norm.weight.min()) == 1.0 and float(m.blocks[0].norm1.bias.abs().sum()) == 0.0


# ---- refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kwargs,exc', [({'init_values': 1e-5}, NotImplementedError), ({'drop_rate': 0.1}, NotImplementedError),
                                        ({'attn_drop_rate': 0.1}, NotImplementedError),
                                        ({'embed_dim': 240}, NotImplementedError),
                                        ({'num_heads': 4}, NotImplementedError),
                                        ({'weight_init': 'jax'}, NotImplementedError),
                                        ({'weight_init': 'moco'}, NotImplementedError),
                                        ({'block_fn': nn.Identity}, NotImplementedError),
                                        ({'img_size': 200}, NotImplementedError),
                                        ({'pretrained': True}, RuntimeError)])
def test_refusals(kwargs, exc):
    with pytest.raises(exc):
        T.BACKBONES.get('vit_tiny_patch16_224')(**kwargs)


def test_head_dim_refusal_of_the_attention_unit(vit_backend):
    from torchok_amd import engine
    from torchok_amd.engine import transformer as ET
    with torch.no_grad(), engine.region() as r:
        x = r.input(torch.randn(2 * 5, 3 * 2 * 32))
        with pytest.raises(NotImplementedError):
            ET.global_attention(r, x, 2, 5, 2, head_dim=32)


# ---- the reference's known answers ---------------------------------------------------------------------------------------------
def test_known_output_shapes_vit_tiny(vit_backend):
    m = T.BACKBONES.get('vit_tiny_patch16_224')().eval()
    x = torch.randn(2, 3, 224, 224)
    with torch.no_grad():
        y = m(x)
        feats = m.forward_features(x)
    assert tuple(y.shape) == (2, 192)
    assert [tuple(f.shape) for f in feats] == [(2, 3, 224, 224)] + [(2, 192, 14, 14)] * 4
    assert 'global_attn_fwd' in vit_backend.calls and 'patch_gather' in vit_backend.calls


@pytest.mark.parametrize('kwargs', [{}, dict(class_token=False), dict(no_embed_class=True),
                                    dict(pre_norm=True, norm_layer=nn.LayerNorm, qkv_bias=False)])
def test_eval_forward_and_features_match_the_restatement(vit_backend, kwargs):
    m = T.BACKBONES.get('vit_tiny_patch16_224')(img_size=48, depth=2, **kwargs).eval()
    ref = ref_state(V.VisionTransformer(img_size=48, patch_size=16, embed_dim=192, depth=2, num_heads=3, **kwargs), 4).eval()
    copy_state(ref, m)
    x = torch.randn(3, 3, 48, 48, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        assert rel_err(m(x).float(), ref(x)) < 3e-2
        mine, want = m.forward_features(x), ref.forward_features(x)
    assert [tuple(f.shape) for f in mine] == [tuple(f.shape) for f in want]
    assert rel_err(mine[1].float(), want[1]) < 3e-2


# ---- training steps against the restatement --------------------------------------------------------------------------------------
STEP_CASES = [('vit_tiny_patch16_224', {}), ('vit_tiny_patch16_224', dict(class_token=False)),
              ('vit_tiny_patch16_224', dict(no_embed_class=True)),
              ('vit_tiny_patch16_224', dict(pre_norm=True, norm_layer=nn.LayerNorm, qkv_bias=False)),
              ('vit_small_patch16_224', {})]


def _ref_kwargs(name, kwargs):
    patch, dim, _, heads, _, _, _ = SERVED[name]
    return dict(patch_size=patch, embed_dim=dim, num_heads=heads, **kwargs)


@pytest.mark.parametrize('name,kwargs', STEP_CASES)
def test_training_step_matches_the_restatement(vit_backend, name, kwargs):
    import oracle.torchok_ref as R
    torch.manual_seed(0)
    bp = dict(img_size=32, depth=2, **kwargs)
    task = vit_task(name, backbone_params=bp)
    ref = ref_state(V.Classifier(10, img_size=32, depth=2, **_ref_kwargs(name, kwargs)), 3)
    copy_state(ref, task)
    task.train()
    ref.train()
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(4, 3, 32, 32, generator=g), torch.randint(0, 10, (4,), generator=g)
    ref2 = copy.deepcopy(ref)
    with torch.autocast('cpu', dtype=torch.bfloat16):
        o = ref2(x)
    F.cross_entropy(o.float(), y).backward()
    out = task.training_step({'image': x, 'target': y}, 0)
    out['loss'].backward()
    logits = ref(x)
    ref_loss = F.cross_entropy(logits, y)
    ref_loss.backward()
    assert abs(float(out['loss']) - float(ref_loss)) < 2e-2 * max(1.0, abs(float(ref_loss)))
    rp, ap = dict(ref.named_parameters()), dict(ref2.named_parameters())
    assert {n for n, _ in task.named_parameters()} == set(rp)
    for n, p in task.named_parameters():
        mine, yard = rel_err(p.grad, rp[n].grad), rel_err(ap[n].grad, rp[n].grad)
        assert mine < 1.5 * yard + 2e-2, (n, mine, yard)
    for what in ('global_attn_fwd', 'global_attn_bwd', 'vit_embed_fwd', 'vit_embed_bwd', 'patch_gather', 'rows_select'):
        assert what in vit_backend.calls, what
    del R


def test_drop_path_with_pinned_draws_matches_the_restatement(vit_backend):
    torch.manual_seed(0)
    task = vit_task('vit_tiny_patch16_224', backbone_params=dict(img_size=32, depth=2, drop_path_rate=0.5))
    dps = [blk.drop_path2 for blk in task.backbone.blocks]
    assert type(task.backbone.blocks[0].drop_path1).__name__ == 'Identity'        # linspace(0, rate, depth)[0] == 0
    assert abs(task.backbone.blocks[1].drop_path1.drop_prob - 0.5) < 1e-7
    ref = ref_state(V.Classifier(10, img_size=32, depth=2, **_ref_kwargs('vit_tiny_patch16_224', {})), 5)
    copy_state(ref, task)
    task.train()
    ref.train()
    s = torch.tensor([2.0, 0.0, 2.0, 0.0])
    t = torch.tensor([0.0, 2.0, 2.0, 0.0])
    blk = task.backbone.blocks[1]
    blk.drop_path1._drawn, blk.drop_path2._drawn = s.clone(), t.clone()
    ref.backbone.blocks[1].drop_scales = (s, t)
    import torchok_amd.models.backbones.vit as vit_mod
    orig = vit_mod.draw_drop_scales
    vit_mod.draw_drop_scales = lambda *a, **k: None            # keep the pinned vectors
    try:
        g = torch.Generator().manual_seed(1)
        x, y = torch.randn(4, 3, 32, 32, generator=g), torch.randint(0, 10, (4,), generator=g)
        out = task.training_step({'image': x, 'target': y}, 0)
        out['loss'].backward()
    finally:
        vit_mod.draw_drop_scales = orig
    ref_loss = F.cross_entropy(ref(x), y)
    ref_loss.backward()
    assert abs(float(out['loss']) - float(ref_loss)) < 2e-2 * max(1.0, abs(float(ref_loss)))
    rp = dict(ref.named_parameters())
    for n, p in task.named_parameters():
        assert rel_err(p.grad, rp[n].grad) < 5e-2, n
    del dps


# ---- frozen stages --------------------------------------------------------------------------------------------------------------
def test_get_stages_holder_quirk_keeps_pos_embed_and_cls_token_trainable(vit_backend):
    task = vit_task('vit_tiny_patch16_224', backbone_params=dict(img_size=32, depth=3))
    bb = task.backbone
    stages = bb.get_stages(2)
    holder = stages[1]
    assert holder.pos_embed is not bb.pos_embed and holder.cls_token is not bb.cls_token
    assert holder.pos_embed.data_ptr() == bb.pos_embed.data_ptr()
    assert list(stages)[4:] == [bb.blocks[0], bb.blocks[1]]
    for p in stages.parameters():
        p.requires_grad_(False)
    assert bb.pos_embed.requires_grad and bb.cls_token.requires_grad           # the reference's quirk
    frozen = list(bb.patch_embed.parameters()) + list(bb.blocks[0].parameters()) + list(bb.blocks[1].parameters())
    task.train()
    g = torch.Generator().manual_seed(1)
    out = task.training_step({'image': torch.randn(2, 3, 32, 32, generator=g), 'target': torch.randint(0, 10, (2,), generator=g)}, 0)
    out['loss'].backward()
    assert all(p.grad is None for p in frozen)
    assert bb.pos_embed.grad is not None and bb.cls_token.grad is not None
    assert all(p.grad is not None for p in bb.blocks[2].parameters())


def test_frozen_pos_embed_and_cls_token_launch_no_fold(vit_backend):
    task = vit_task('vit_tiny_patch16_224', backbone_params=dict(img_size=32, depth=1))
    bb = task.backbone
    bb.pos_embed.requires_grad_(False)
    task.train()
    out = task.training_step({'image': torch.randn(2, 3, 32, 32), 'target': torch.randint(0, 10, (2,))}, 0)
    out['loss'].backward()
    assert bb.pos_embed.grad is None and bb.cls_token.grad is not None
    assert 'vit_embed_dpos' not in vit_backend.calls and 'vit_embed_dcls' in vit_backend.calls
    bb.cls_token.requires_grad_(False)
    vit_backend.calls.clear()
    out = task.training_step({'image': torch.randn(2, 3, 32, 32), 'target': torch.randint(0, 10, (2,))}, 0)
    out['loss'].backward()
    assert 'vit_embed_bwd' not in vit_backend.calls


# ---- the recipe through the fit loop --------------------------------------------------------------------------------------------
def test_vit_recipe_through_the_fit_loop(vit_backend):
    from torchok_amd.run import fit
    os.environ.setdefault('HOME', '/root')
    cfg = T.load_config(os.path.join(RECIPES, 'classification_vit.yaml'),
                        overrides={'task.params.backbone_params.img_size': 32, 'task.params.backbone_params.depth': 2,
                                   'trainer.devices': 1})
    assert cfg.task.params.backbone_name == 'vit_tiny_patch16_224' and cfg.task.params.get('pooling_name') is None
    torch.manual_seed(0)
    seen = []
    batches = [{'image': torch.randn(4, 3, 32, 32), 'target': torch.randint(0, 10, (4,))} for _ in range(2)]
    res = fit(cfg, batches=batches, max_steps=2, device='cpu', on_step=lambda i, out: seen.append(float(out['loss'])))
    assert res['steps'] == 2 and len(seen) == 2 and all(v == v for v in seen)
    assert 'global_attn_bwd' in vit_backend.calls
