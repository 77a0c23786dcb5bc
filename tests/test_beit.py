"""BEiT backbones (torchok_amd/models/backbones/beit.py) on the host-memory stand-in of the library: the biased global-attention,
relative-position-bias and LayerScale entry points (and the ViT ones BEiT shares) are written here in torch, over the same
layouts the kernels use.  Registration and parameter counts, the timm state_dict layout, initialisation facts, the refusals, a
training step against the plain-torch restatement (tests/beit_ref.py) and run.fit over the recipe."""
import copy
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import beit_ref as R
import fake_backend as fb
import torchok_amd as T
from helpers import rel_err

RECIPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'recipes')
BF, F32, I64 = torch.bfloat16, torch.float32, torch.int64

# name -> (embed_dim, depth, heads, img_size, init_values, parameters): 12 d^2 + 13 d + 2 d (gammas) + T heads per block,
# patch embedding, cls token, final norm and the FPN containers (3 transposed convolutions + one BatchNorm)
ENTRIES = {
    'beit_base_patch16_224': (768, 12, 12, 224, 0.1), 'beit_base_patch16_384': (768, 12, 12, 384, 0.1),
    'beit_base_patch16_224_in22k': (768, 12, 12, 224, 0.1), 'beit_large_patch16_224': (1024, 24, 16, 224, 1e-5),
    'beit_large_patch16_384': (1024, 24, 16, 384, 1e-5), 'beit_large_patch16_512': (1024, 24, 16, 512, 1e-5),
    'beit_large_patch16_224_in22k': (1024, 24, 16, 224, 1e-5),
}


def _count(dim, depth, heads, img):
    g = img // 16
    table = ((2 * g - 1) ** 2 + 3) * heads
    block = (3 * dim * dim + 2 * dim) + (dim * dim + dim) + (8 * dim * dim + 5 * dim) + 4 * dim + 2 * dim + table
    fpn = 3 * (4 * dim * dim + dim) + 2 * dim
    return depth * block + (3 * 256 * dim + dim) + dim + 2 * dim + fpn


class BeitFake(fb.FakeTok):
    """FakeTok plus the entry points of include/tok.h that BEiT reaches: tok_global_attn_*, tok_global_attn_bias_*,
    tok_relpos_bias_*, tok_layer_scale_*, tok_patch_gather, tok_vit_embed_* and tok_rows_select."""

    def _attn(self, qkv, ldq, b, n, heads, bias):
        c = heads * 64
        x = fb._t(qkv, (b, n, ldq), BF)[..., :3 * c].float().clone().requires_grad_(True)
        q, k, v = x.reshape(b, n, 3, heads, 64).permute(2, 0, 3, 1, 4)
        s = (q @ k.transpose(-2, -1)) * 0.125
        if bias is not None:
            s = s + bias.unsqueeze(0)
        return x, s, (s.softmax(-1) @ v).transpose(1, 2).reshape(b, n, c)

    def _fwd(self, qkv, ldq, b, n, heads, head_dim, out, ldo, lse, bias):
        if head_dim != 64:
            self._err = b'head_dim not served'
            return -1
        with torch.no_grad():
            _, s, o = self._attn(qkv, ldq, b, n, heads, bias)
        fb._t(lse, (b, heads, n), F32).copy_(torch.logsumexp(s, -1))
        fb._t(out, (b, n, ldo), BF)[..., :heads * 64] = o.to(BF)
        return 0

    def tok_global_attn_fwd(self, qkv, ldq, b, n, heads, head_dim, out, ldo, lse, st):
        self.calls.append('global_attn_fwd')
        return self._fwd(qkv, ldq, b, n, heads, head_dim, out, ldo, lse, None)

    def tok_global_attn_bias_fwd(self, qkv, ldq, bias, ldb, b, n, heads, head_dim, out, ldo, lse, st):
        self.calls.append('global_attn_bias_fwd')
        assert ldb >= n and ldb % 4 == 0
        return self._fwd(qkv, ldq, b, n, heads, head_dim, out, ldo, lse, fb._t(bias, (heads, n, ldb), F32)[..., :n])

    def tok_global_attn_bwd_ws_bytes(self, b, n, heads):
        return 4 * b * n * heads

    def tok_global_attn_bias_bwd_ws_bytes(self, b, n, heads, ldb):
        return 4 * b * n * heads + 4 * heads * n * ldb

    def tok_global_attn_bwd(self, qkv, ldq, out, dout, ldo, lse, b, n, heads, head_dim, dqkv, ldd, ws, ws_bytes, st):
        self.calls.append('global_attn_bwd')
        c = heads * 64
        with torch.enable_grad():
            x, _, o = self._attn(qkv, ldq, b, n, heads, None)
            g, = torch.autograd.grad(o, x, fb._t(dout, (b, n, ldo), BF)[..., :c].float())
        fb._t(dqkv, (b, n, ldd), BF)[..., :3 * c] = g.to(BF)
        return 0

    def tok_global_attn_bias_bwd(self, qkv, ldq, out, dout, ldo, lse, bias, ldb, b, n, heads, head_dim, dqkv, ldd, dbias, dbias_acc,
                                 ws, ws_bytes, st):
        self.calls.append('global_attn_bias_bwd')
        c = heads * 64
        bs = fb._t(bias, (heads, n, ldb), F32)[..., :n].clone().requires_grad_(True)
        with torch.enable_grad():
            x, _, o = self._attn(qkv, ldq, b, n, heads, bs)
            g, gb = torch.autograd.grad(o, (x, bs), fb._t(dout, (b, n, ldo), BF)[..., :c].float())
        fb._t(dqkv, (b, n, ldd), BF)[..., :3 * c] = g.to(BF)
        if dbias is not None:
            self.calls.append('global_attn_dbias')
            t = fb._t(dbias, (heads, n, ldb), F32)
            t[..., :n] = gb + t[..., :n] if dbias_acc else gb
        return 0

    def tok_relpos_bias_fwd(self, table, index, heads, n, bias, ldb, st):
        self.calls.append('relpos_bias_fwd')
        idx = fb._t(index, (n * n,), I64)
        tab = fb._t(table, (int(idx.max()) + 1, heads), F32)
        fb._t(bias, (heads, n, ldb), F32)[..., :n] = tab[idx].view(n, n, heads).permute(2, 0, 1)
        return 0

    def tok_relpos_bias_bwd(self, dbias, ldb, index, heads, n, rows, dtable, accumulate, st):
        self.calls.append('relpos_bias_bwd')
        idx = fb._t(index, (n * n,), I64)
        g = fb._t(dbias, (heads, n, ldb), F32)[..., :n].permute(1, 2, 0).reshape(n * n, heads)
        t = fb._t(dtable, (rows, heads), F32)
        v = torch.zeros(rows, heads).index_add_(0, idx, g)
        t.copy_(v + t if accumulate else v)
        return 0

    @staticmethod
    def _scale(row_scale, rps, rows):
        if row_scale is None:
            return torch.ones(rows, 1)
        return fb._t(row_scale, ((rows + rps - 1) // rps,), F32).repeat_interleave(rps)[:rows, None]

    def tok_layer_scale_fwd(self, x, a, gamma, row_scale, rps, out, rows, d, st):
        self.calls.append('layer_scale_fwd')
        v = fb._t(x, (rows, d), BF).float() + self._scale(row_scale, rps, rows) * fb._t(gamma, (d,), F32) * fb._t(a, (rows, d), BF).float()
        fb._t(out, (rows, d), BF).copy_(v.to(BF))
        return 0

    def tok_layer_scale_bwd_rows(self, rows, d):
        return 1

    def tok_layer_scale_bwd(self, dout, a, gamma, row_scale, rps, da, da_acc, dgamma, dg_acc, partial, rows, d, st):
        self.calls.append('layer_scale_bwd')
        g = fb._t(dout, (rows, d), BF).float() * self._scale(row_scale, rps, rows)
        if da is not None:
            t = fb._t(da, (rows, d), BF)
            v = g * fb._t(gamma, (d,), F32)
            t.copy_((v + t.float() if da_acc else v).to(BF))
        if dgamma is not None:
            self.calls.append('layer_scale_dgamma')
            t = fb._t(dgamma, (d,), F32)
            v = (g * fb._t(a, (rows, d), BF).float()).sum(0)
            t.copy_(v + t if dg_acc else v)
        return 0

    def tok_patch_gather(self, img, n, h, w, p, rows, st):
        self.calls.append('patch_gather')
        x = fb._t(img, (n, h // p, p, w // p, p, 4), BF)
        fb._t(rows, (n, h // p, w // p, p, p, 4), BF).copy_(x.permute(0, 1, 3, 2, 4, 5))
        return 0

    def tok_vit_embed_fwd(self, patch, pos, cls, b, n_p, d, no_embed_class, out, st):
        self.calls.append('vit_embed_fwd')
        assert cls is not None and not no_embed_class
        x = torch.cat((fb._t(cls, (1, 1, d), F32).expand(b, -1, -1), fb._t(patch, (b, n_p, d), BF).float()), 1)
        fb._t(out, (b, n_p + 1, d), BF).copy_((x + fb._t(pos, (n_p + 1, d), F32)).to(BF))
        return 0

    def tok_vit_embed_bwd(self, dout, b, n_p, d, has_cls, no_embed_class, dpos, pos_acc, dcls, cls_acc, st):
        self.calls.append('vit_embed_bwd')
        g = fb._t(dout, (b, n_p + 1, d), BF).float()
        if dpos is not None:
            self.calls.append('vit_embed_dpos')
            t = fb._t(dpos, (n_p + 1, d), F32)
            t.copy_(g.sum(0) + t if pos_acc else g.sum(0))
        if dcls is not None:
            t = fb._t(dcls, (d,), F32)
            t.copy_(g[:, 0].sum(0) + t if cls_acc else g[:, 0].sum(0))
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
def beit_backend():
    token = fb.install(BeitFake())
    yield token[0]
    fb.uninstall(token)


# ---- registration and layout -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_every_entry_point_constructs_with_the_reference_parameter_count(name):
    dim, depth, heads, img, init_values = ENTRIES[name]
    with torch.device('meta'):
        m = T.BACKBONES.get(name)(pretrained=False, in_channels=3)
    assert type(m).__name__ == 'Beit' and m.out_channels == dim and m.num_features == dim
    assert m.out_encoder_channels == (dim,) * 4 and m.out_indices == (3, 5, 7, 11)
    assert m.img_size == (img, img) and m.patch_embed.patch_size == (16, 16)
    assert len(m.blocks) == depth and m.blocks[0].attn.num_heads == heads
    assert m.pos_embed is None and m.rel_pos_bias is None
    g = img // 16
    assert tuple(m.blocks[-1].attn.relative_position_bias_table.shape) == ((2 * g - 1) ** 2 + 3, heads)
    assert tuple(m.blocks[-1].attn.relative_position_index.shape) == (g * g + 1, g * g + 1)
    assert sum(p.numel() for p in m.parameters()) == _count(dim, depth, heads, img)


def test_parameter_count_of_the_base_model_is_the_published_one_plus_the_fpn():
    # timm's beit_base_patch16_224 without its 1000-class head has 85 761 984 parameters (86 530 984 - 769 000); the reference
    # adds the FPN containers
    fpn = 3 * (4 * 768 * 768 + 768) + 2 * 768
    assert _count(768, 12, 12, 224) - fpn == 85761984


def test_state_dict_keys_of_beit_base():
    with torch.device('meta'):
        m = T.BACKBONES.get('beit_base_patch16_224')()
    keys = set(m.state_dict())
    per_block = {'gamma_1', 'gamma_2', 'norm1.weight', 'norm1.bias', 'attn.q_bias', 'attn.v_bias',
                 'attn.relative_position_bias_table', 'attn.relative_position_index', 'attn.qkv.weight', 'attn.proj.weight',
                 'attn.proj.bias', 'norm2.weight', 'norm2.bias', 'mlp.fc1.weight', 'mlp.fc1.bias', 'mlp.fc2.weight', 'mlp.fc2.bias'}
    want = {'cls_token', 'patch_embed.proj.weight', 'patch_embed.proj.bias', 'norm.weight', 'norm.bias', 'fpn1.0.weight',
            'fpn1.0.bias', 'fpn1.1.weight', 'fpn1.1.bias', 'fpn1.1.running_mean', 'fpn1.1.running_var',
            'fpn1.1.num_batches_tracked', 'fpn1.3.weight', 'fpn1.3.bias', 'fpn2.weight', 'fpn2.bias'}
    want |= {f'blocks.{i}.{k}' for i in range(12) for k in per_block}
    assert keys == want
    assert not any('k_bias' in k for k in keys) and 'pos_embed' not in keys
    assert m.blocks[0].attn.k_bias is not None and tuple(m.state_dict()['fpn1.0.weight'].shape) == (768, 768, 2, 2)


def test_state_dict_interchanges_with_the_restatement():
    m = T.BACKBONES.get('beit_base_patch16_224')(**R.TINY_BP)
    ref = R.Beit(**R.TINY)
    mine = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith('fpn')}
    assert mine == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    m2 = T.BACKBONES.get('beit_base_patch16_224')(use_abs_pos_emb=True, init_values=None, use_rel_pos_bias=False, qkv_bias=False,
                                                  **R.TINY_BP)
    ref2 = R.Beit(**dict(R.TINY, use_abs_pos_emb=True, init_values=None, use_rel_pos_bias=False, qkv_bias=False))
    mine = {k: tuple(v.shape) for k, v in m2.state_dict().items() if not k.startswith('fpn')}
    assert mine == {k: tuple(v.shape) for k, v in ref2.state_dict().items()} and 'pos_embed' in mine


def test_init_facts():
    torch.manual_seed(0)
    m = T.BACKBONES.get('beit_base_patch16_224')(depth=4, use_abs_pos_emb=True)
    for blk in m.blocks:
        assert float(blk.attn.relative_position_bias_table.detach().abs().sum()) == 0.0
        assert torch.equal(blk.gamma_1.detach(), torch.full((768,), 0.1)) and torch.equal(blk.gamma_2.detach(), torch.full((768,), 0.1))
        assert float(blk.attn.q_bias.detach().abs().sum()) == 0.0 and float(blk.mlp.fc1.bias.detach().abs().sum()) == 0.0
    std = lambda w: float(w.detach().std())        # noqa: E731
    assert abs(std(m.blocks[0].attn.qkv.weight) - 0.02) < 1e-3
    # fix_init_weight: proj / fc2 of layer l divided by sqrt(2 l): layers 1 and 4 differ by sqrt(8 / 2) = 2
    assert abs(std(m.blocks[0].attn.proj.weight) / std(m.blocks[3].attn.proj.weight) - 2.0) < 0.02
    assert abs(std(m.blocks[0].mlp.fc2.weight) / std(m.blocks[3].mlp.fc2.weight) - 2.0) < 0.02
    assert abs(std(m.blocks[0].attn.proj.weight) - 0.02 / 2 ** 0.5) < 1e-3
    assert abs(std(m.cls_token) - 0.02) < 3e-3 and abs(std(m.pos_embed) - 0.02) < 1e-3
    assert float(m.norm.weight.min()) == 1.0 and float(m.blocks[0].norm1.bias.abs().sum()) == 0.0
    large = T.BACKBONES.get('beit_large_patch16_224')(depth=1)
    assert torch.equal(large.blocks[0].gamma_1.detach(), torch.full((1024,), 1e-5))


def test_no_weight_decay_and_get_stages():
    m = T.BACKBONES.get('beit_base_patch16_224')(**R.TINY_BP)
    assert m.no_weight_decay() == {'pos_embed', 'cls_token', 'blocks.0.attn.relative_position_bias_table',
                                   'blocks.1.attn.relative_position_bias_table'}
    assert m.get_stages(2) is m


# ---- refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kwargs,exc', [({'use_shared_rel_pos_bias': True}, NotImplementedError),
                                        ({'drop_rate': 0.1}, NotImplementedError), ({'attn_drop_rate': 0.1}, NotImplementedError),
                                        ({'embed_dim': 240}, NotImplementedError), ({'num_heads': 4}, NotImplementedError),
                                        ({'norm_layer': nn.BatchNorm1d}, NotImplementedError),
                                        ({'img_size': 200}, NotImplementedError), ({'pretrained': True}, RuntimeError)])
def test_refusals(kwargs, exc):
    with pytest.raises(exc):
        T.BACKBONES.get('beit_base_patch16_224')(**dict(dict(depth=1), **kwargs))


def test_forward_features_is_refused():
    m = T.BACKBONES.get('beit_base_patch16_224')(**R.TINY_BP)
    with pytest.raises(NotImplementedError):
        m.forward_features(torch.randn(1, 3, 64, 64))


def test_index_outside_the_table_is_refused_on_the_host(beit_backend):
    from torchok_amd import engine
    from torchok_amd.engine import transformer as ET
    table = nn.Parameter(torch.zeros(12, 2))
    index = R.gen_relative_position_index((2, 2))
    with torch.no_grad(), engine.region() as r:
        ET.relpos_bias(r, table, index, 2, 5)
        for v in (12, -1):
            bad = index.clone()
            bad[4, 1] = v
            with pytest.raises(ValueError):
                ET.relpos_bias(r, table, bad, 2, 5)
    assert beit_backend.calls.count('relpos_bias_fwd') == 1


# ---- forward and training steps against the restatement ----------------------------------------------------------------------
def _task_and_ref(bp=None, seed=3, **kw):
    bp = bp or {}
    task = R.beit_task(backbone_params=dict(R.TINY_BP, **bp), **kw)
    ref_kw = {k: v for k, v in bp.items() if k != 'drop_path_rate'}
    ref = R.ref_state(R.Classifier(10, **dict(R.TINY, **ref_kw)), seed)
    R.copy_backbone_state(ref, task)
    return task, ref


def test_eval_forward_matches_the_restatement(beit_backend):
    task, ref = _task_and_ref(seed=4)
    task.eval()
    ref.eval()
    x = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        y = task.backbone(x)
        assert tuple(y.shape) == (3, 128, 1, 1)
        assert rel_err(y.float(), ref.backbone(x)) < 3e-2
    assert 'global_attn_bias_fwd' in beit_backend.calls and 'global_attn_fwd' not in beit_backend.calls


@pytest.mark.parametrize('bp', [{}, dict(use_abs_pos_emb=True), dict(init_values=None), dict(qkv_bias=False, use_rel_pos_bias=False)],
                         ids=['default', 'abs_pos', 'no_layer_scale', 'no_bias'])
def test_training_step_matches_the_restatement(beit_backend, bp):
    torch.manual_seed(0)
    task, ref = _task_and_ref(bp)
    task.train()
    ref.train()
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(4, 3, 64, 64, generator=g), torch.randint(0, 10, (4,), generator=g)
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
        if n.startswith('backbone.fpn'):
            assert p.grad is None, n
            continue
        mine, yard = rel_err(p.grad, rp[n].grad), rel_err(ap[n].grad, rp[n].grad)
        assert mine < 1.5 * yard + 2e-2, (n, mine, yard)
        seen.add(n)
    assert seen == set(rp)
    calls = beit_backend.calls
    biased = bp.get('use_rel_pos_bias', True)
    for what in (('global_attn_bias_fwd', 'global_attn_bias_bwd', 'global_attn_dbias', 'relpos_bias_bwd') if biased else
                 ('global_attn_fwd', 'global_attn_bwd')):
        assert what in calls, what
    # the bias is gathered once per block in the forward and once more in the backward: no block keeps it
    assert calls.count('relpos_bias_fwd') == (4 if biased else 0)
    assert ('layer_scale_dgamma' in calls) == (bp.get('init_values', 0.1) is not None)
    assert ('vit_embed_dpos' in calls) == bool(bp.get('use_abs_pos_emb'))


def test_frozen_table_and_gammas_take_no_gradient(beit_backend):
    task, _ = _task_and_ref()
    for n, p in task.named_parameters():
        if 'relative_position_bias_table' in n or 'gamma' in n:
            p.requires_grad_(False)
    task.train()
    out = task.training_step({'image': torch.randn(2, 3, 64, 64), 'target': torch.randint(0, 10, (2,))}, 0)
    out['loss'].backward()
    for n, p in task.named_parameters():
        if 'relative_position_bias_table' in n or 'gamma' in n:
            assert p.grad is None, n
    calls = beit_backend.calls
    assert 'global_attn_bias_bwd' in calls and 'global_attn_dbias' not in calls and 'relpos_bias_bwd' not in calls
    assert 'layer_scale_bwd' in calls and 'layer_scale_dgamma' not in calls


def test_drop_path_with_pinned_draws_matches_the_restatement(beit_backend):
    import torchok_amd.models.backbones.beit as beit_mod
    torch.manual_seed(0)
    task, ref = _task_and_ref(dict(drop_path_rate=0.5), seed=5)
    assert type(task.backbone.blocks[0].drop_path1).__name__ == 'Identity'        # linspace(0, rate, depth)[0] == 0
    assert abs(task.backbone.blocks[1].drop_path2.drop_prob - 0.5) < 1e-7
    task.train()
    ref.train()
    s, t = torch.tensor([2.0, 0.0, 2.0, 0.0]), torch.tensor([0.0, 2.0, 2.0, 0.0])
    blk = task.backbone.blocks[1]
    blk.drop_path1._drawn, blk.drop_path2._drawn = s.clone(), t.clone()
    ref.backbone.blocks[1].drop_scales = (s, t)
    orig = beit_mod.draw_drop_scales
    beit_mod.draw_drop_scales = lambda *a, **k: None            # keep the pinned vectors
    try:
        g = torch.Generator().manual_seed(1)
        x, y = torch.randn(4, 3, 64, 64, generator=g), torch.randint(0, 10, (4,), generator=g)
        out = task.training_step({'image': x, 'target': y}, 0)
        out['loss'].backward()
    finally:
        beit_mod.draw_drop_scales = orig
    ref_loss = F.cross_entropy(ref(x), y)
    ref_loss.backward()
    assert abs(float(out['loss']) - float(ref_loss)) < 2e-2 * max(1.0, abs(float(ref_loss)))
    rp = dict(ref.named_parameters())
    for n, p in task.named_parameters():
        if not n.startswith('backbone.fpn'):
            assert rel_err(p.grad, rp[n].grad) < 5e-2, n


# ---- the recipe through the fit loop --------------------------------------------------------------------------------------------
def test_beit_recipe_through_the_fit_loop(beit_backend):
    from torchok_amd.run import fit
    os.environ.setdefault('HOME', '/root')
    cfg = T.load_config(os.path.join(RECIPES, 'classification_beit.yaml'), overrides={'trainer.devices': 1})
    assert cfg.task.params.backbone_name == 'beit_base_patch16_224' and cfg.task.params.pooling_name == 'Pooling'
    assert cfg.optimization[0].optimizer.name == 'AdamW'
    torch.manual_seed(0)
    seen = []
    batches = [{'image': torch.randn(4, 3, 64, 64), 'target': torch.randint(0, 10, (4,))} for _ in range(2)]
    res = fit(cfg, batches=batches, max_steps=2, device='cpu', on_step=lambda i, out: seen.append(float(out['loss'])))
    assert res['steps'] == 2 and len(seen) == 2 and all(v == v for v in seen)
    assert 'global_attn_bias_bwd' in beit_backend.calls and 'layer_scale_bwd' in beit_backend.calls
