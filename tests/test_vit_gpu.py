"""Vision Transformer on the MI355X: the global-attention kernels against fp64 torch on the same bf16 inputs (every token
count from 1 to 1025, unaligned row pitches, bit-identical reruns), the embedding kernels against torch, ClassificationTask
steps against the fp32 restatement (tests/vit_ref.py) within the bf16-autocast yardstick of test_resnet_gpu.py,
reproducibility and hipGraph replay."""
import copy

import pytest
import torch
import torch.nn.functional as F

import vit_ref as V
from helpers import copy_state, rel_err
from test_vit import SERVED, ref_state, vit_task
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
p_ = lambda t: None if t is None else t.data_ptr()     # noqa: E731


def _attn(qkv, b, n, heads, ldo, dout):
    lib = _C.lib()
    c = heads * 64
    out = torch.zeros((b * n, ldo), dtype=BF, device='cuda')
    lse = torch.empty((b, heads, n), dtype=torch.float32, device='cuda')
    _C.check(lib.tok_global_attn_fwd(p_(qkv), qkv.shape[1], b, n, heads, 64, p_(out), ldo, p_(lse), stream_ptr()), 'fwd')
    dqkv = torch.full_like(qkv, 7.0)
    ws_bytes = lib.tok_global_attn_bwd_ws_bytes(b, n, heads)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device='cuda')
    _C.check(lib.tok_global_attn_bwd(p_(qkv), qkv.shape[1], p_(out), p_(dout), ldo, p_(lse), b, n, heads, 64, p_(dqkv),
                                     qkv.shape[1], p_(ws), ws_bytes, stream_ptr()), 'bwd')
    torch.cuda.synchronize()
    return out[:, :c], lse, dqkv


@pytest.mark.parametrize('n', [1, 17, 50, 64, 65, 197, 257, 577, 785, 1025])
@pytest.mark.parametrize('b,heads', [(2, 3), (1, 6)])
def test_global_attention_vs_fp64(n, b, heads):
    c = heads * 64
    ldq, ldo = 3 * c + 8, c + 24                    # pitches wider than the rows: the kernels must honour them
    g = torch.Generator().manual_seed(n * 7 + heads)
    qkv = (torch.randn(b * n, ldq, generator=g) * 1.5).to(BF)
    dout = torch.zeros(b * n, ldo).to(BF)
    dout[:, :c] = torch.randn(b * n, c, generator=g).to(BF)
    x = qkv[:, :3 * c].double().requires_grad_(True)
    q, k, v = x.reshape(b, n, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * 0.125
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(b * n, c)
    o.backward(dout[:, :c].double())
    out, lse, dqkv = _attn(qkv.cuda(), b, n, heads, ldo, dout.cuda())
    assert rel_err(out.cpu(), o) < 1e-2
    assert (lse.cpu().double() - torch.logsumexp(s, -1)).abs().max() < 1e-3
    dq = dqkv.cpu()
    floor = 1e-2 * float(x.grad.norm())             # with one token dq = dk = 0 exactly: measure against the whole gradient
    for i, what in enumerate(('dq', 'dk', 'dv')):
        want = x.grad[:, i * c:(i + 1) * c]
        e = float((dq[:, i * c:(i + 1) * c].double() - want).norm()) / max(float(want.norm()), floor)
        assert e < 2e-2, (what, e)
    assert torch.all(dq[:, 3 * c:] == 7.0)          # the pad columns of d(qkv) are not the kernel's
    out2, lse2, dqkv2 = _attn(qkv.cuda(), b, n, heads, ldo, dout.cuda())
    assert torch.equal(out, out2) and torch.equal(lse, lse2) and torch.equal(dqkv, dqkv2)


@pytest.mark.parametrize('head_dim', [32, 80])
def test_head_dim_refusal(head_dim):
    lib = _C.lib()
    qkv = torch.zeros((4, 3 * 64), dtype=BF, device='cuda')
    out = torch.zeros((4, 64), dtype=BF, device='cuda')
    lse = torch.zeros(4, dtype=torch.float32, device='cuda')
    rc = lib.tok_global_attn_fwd(p_(qkv), 3 * head_dim, 1, 4, 1, head_dim, p_(out), head_dim, p_(lse), stream_ptr())
    assert rc == -1 and b'head_dim' in lib.tok_last_error()
    rc = lib.tok_global_attn_fwd(p_(qkv), 192, 1, 5000, 1, 64, p_(out), 64, p_(lse), stream_ptr())
    assert rc == -1


@pytest.mark.parametrize('p,h,w', [(16, 32, 48), (14, 28, 28), (8, 16, 8), (32, 64, 32)])
def test_patch_gather(p, h, w):
    lib = _C.lib()
    img = torch.randn(3, h, w, 4).to(BF).cuda()
    rows = torch.empty((3 * (h // p) * (w // p), p * p * 4), dtype=BF, device='cuda')
    _C.check(lib.tok_patch_gather(p_(img), 3, h, w, p, p_(rows), stream_ptr()), 'gather')
    torch.cuda.synchronize()
    want = img.view(3, h // p, p, w // p, p, 4).permute(0, 1, 3, 2, 4, 5).reshape(rows.shape)
    assert torch.equal(rows, want)


@pytest.mark.parametrize('has_cls,no_embed_class', [(True, False), (True, True), (False, False)])
@pytest.mark.parametrize('frozen', ['', 'pos', 'cls'])
def test_vit_embed_kernels(has_cls, no_embed_class, frozen):
    lib = _C.lib()
    b, n_p, d = 5, 49, 192
    prefix = 1 if has_cls else 0
    g = torch.Generator().manual_seed(3)
    patch = torch.randn(b * n_p, d, generator=g).to(BF)
    pos = torch.randn(n_p if no_embed_class else n_p + prefix, d, generator=g)
    cls = torch.randn(d, generator=g) if has_cls else None
    x = patch.float().view(b, n_p, d)
    if no_embed_class:
        x = x + pos
        want = torch.cat((cls.expand(b, 1, d), x), 1) if has_cls else x
    else:
        want = (torch.cat((cls.expand(b, 1, d), x), 1) if has_cls else x) + pos
    out = torch.empty((b * (n_p + prefix), d), dtype=BF, device='cuda')
    patch_d, pos_d, cls_d = patch.cuda(), pos.cuda(), cls.cuda() if has_cls else None     # (kept alive across the launches)
    _C.check(lib.tok_vit_embed_fwd(p_(patch_d), p_(pos_d), p_(cls_d), b, n_p, d,
                                   int(no_embed_class), p_(out), stream_ptr()), 'fwd')
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want.reshape(-1, d).to(BF))
    dout = torch.randn(b, n_p + prefix, d, generator=g).to(BF)
    dpos = torch.full_like(pos, 3.0).cuda() if frozen != 'pos' else None
    dcls = torch.full((d,), 3.0).cuda() if (has_cls and frozen != 'cls') else None
    dout_d = dout.cuda()
    _C.check(lib.tok_vit_embed_bwd(p_(dout_d), b, n_p, d, prefix, int(no_embed_class), p_(dpos), 1, p_(dcls), 0,
                                   stream_ptr()), 'bwd')
    torch.cuda.synchronize()
    gd = dout.double()
    if dpos is not None:
        wp = (gd[:, prefix:] if no_embed_class else gd).sum(0) + 3.0                    # accumulate
        assert (dpos.cpu().double() - wp).abs().max() < 1e-4
    if dcls is not None:
        assert (dcls.cpu().double() - gd[:, 0].sum(0)).abs().max() < 1e-4              # overwrite
    dpatch = torch.empty((b * n_p, d), dtype=BF, device='cuda')
    _C.check(lib.tok_rows_select(p_(dout_d), b, n_p + prefix, prefix, n_p, d, p_(dpatch), 0, 0, stream_ptr()), 'sel')
    back = torch.full((b * (n_p + prefix), d), 5.0, dtype=BF, device='cuda')
    _C.check(lib.tok_rows_select(p_(dpatch), b, n_p + prefix, prefix, n_p, d, p_(back), 1, 0, stream_ptr()), 'sel_t')
    torch.cuda.synchronize()
    assert torch.equal(dpatch.cpu(), dout[:, prefix:].reshape(-1, d))
    want_back = dout.clone()
    want_back[:, :prefix] = 0
    assert torch.equal(back.cpu(), want_back.reshape(-1, d))


# ---- ClassificationTask steps against the restatement ------------------------------------------------------------------------
def _task_and_ref(name, bp, optimizer='SGD', seed=3, classes=10):
    patch, dim, _, heads, _, _, _ = SERVED[name]
    opt = {'SGD': None, 'AdamW': {'lr': 1e-3, 'weight_decay': 0.05}}[optimizer]
    task = vit_task(name, backbone_params=bp, optimizer=optimizer, opt_params=opt, num_classes=classes)
    ref_kw = {k: v for k, v in bp.items() if k != 'drop_path_rate'}
    ref = ref_state(V.Classifier(classes, patch_size=patch, embed_dim=dim, num_heads=heads, **ref_kw), seed)
    copy_state(ref, task)
    return task, ref


@pytest.mark.parametrize('name,optimizer,bp', [
    ('vit_tiny_patch16_224', 'SGD', dict(img_size=224, depth=4)),
    ('vit_tiny_patch16_224', 'AdamW', dict(img_size=224, depth=4, class_token=False)),
    ('vit_small_patch16_224', 'SGD', dict(img_size=224, depth=4, no_embed_class=True)),
    ('vit_small_patch16_224', 'AdamW', dict(img_size=224, depth=4, qkv_bias=False)),
])
def test_training_step_vs_restatement(name, optimizer, bp):
    torch.manual_seed(0)
    task, ref = _task_and_ref(name, bp, optimizer)
    task.cuda().train()
    ref.train()
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(8, 3, 224, 224, generator=g), torch.randint(0, 10, (8,), generator=g)
    ref2 = copy.deepcopy(ref)
    with torch.autocast('cpu', dtype=torch.bfloat16):
        ac_loss = F.cross_entropy(ref2(x).float(), y)
    ac_loss.backward()
    opt = task.configure_optimizers()[0]['optimizer']
    out = task.training_step({'image': x.cuda(), 'target': y.cuda()}, 0)
    out['loss'].backward()
    ref_loss = F.cross_entropy(ref(x), y)
    ref_loss.backward()
    torch.cuda.synchronize()
    assert abs(float(out['loss']) - float(ref_loss)) < max(2e-2, 1.5 * abs(float(ac_loss) - float(ref_loss)) + 1e-2)
    rp, ap = dict(ref.named_parameters()), dict(ref2.named_parameters())
    for n, p in task.named_parameters():
        assert p.grad is not None, n
        mine, yard = rel_err(p.grad, rp[n].grad), rel_err(ap[n].grad, rp[n].grad)
        assert mine < 1.5 * yard + 1e-2, (n, mine, yard)
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in task.parameters())


def test_pre_norm_eval_forward_vs_restatement():
    from torch import nn
    bp = dict(img_size=224, depth=3, pre_norm=True, norm_layer=nn.LayerNorm)
    task, ref = _task_and_ref('vit_base_patch32_224_clip_laion2b', bp, seed=4)
    task.cuda().eval()
    ref.eval()
    x = torch.randn(4, 3, 224, 224, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        mine = task.backbone(x.cuda()).float().cpu()
        want = ref.backbone(x)
        with torch.autocast('cpu', dtype=torch.bfloat16):
            ac = ref.backbone(x).float()
        feats = task.backbone.forward_features(x.cuda())
        want_feats = ref.backbone.forward_features(x)
    assert rel_err(mine, want) < 1.5 * rel_err(ac, want) + 1e-2
    assert [tuple(f.shape) for f in feats] == [tuple(f.shape) for f in want_feats]
    assert rel_err(feats[1].float().cpu(), want_feats[1]) < 5e-2


def test_drop_path_with_pinned_draws_vs_restatement():
    import torchok_amd.models.backbones.vit as vit_mod
    torch.manual_seed(0)
    task, ref = _task_and_ref('vit_tiny_patch16_224', dict(img_size=224, depth=2, drop_path_rate=0.1), seed=5)
    task.cuda().train()
    ref.train()
    s1, s2 = torch.tensor([1 / 0.9, 0.0, 1 / 0.9, 1 / 0.9]), torch.tensor([0.0, 1 / 0.9, 1 / 0.9, 0.0])
    blk = task.backbone.blocks[1]
    blk.drop_path1._drawn, blk.drop_path2._drawn = s1.cuda(), s2.cuda()
    ref.backbone.blocks[1].drop_scales = (s1, s2)
    orig = vit_mod.draw_drop_scales
    vit_mod.draw_drop_scales = lambda *a, **k: None
    try:
        g = torch.Generator().manual_seed(1)
        x, y = torch.randn(4, 3, 224, 224, generator=g), torch.randint(0, 10, (4,), generator=g)
        out = task.training_step({'image': x.cuda(), 'target': y.cuda()}, 0)
        out['loss'].backward()
    finally:
        vit_mod.draw_drop_scales = orig
    ref2 = copy.deepcopy(ref)
    with torch.autocast('cpu', dtype=torch.bfloat16):
        F.cross_entropy(ref2(x).float(), y).backward()
    ref_loss = F.cross_entropy(ref(x), y)
    ref_loss.backward()
    torch.cuda.synchronize()
    assert abs(float(out['loss']) - float(ref_loss)) < 2e-2 * max(1.0, abs(float(ref_loss)))
    rp, ap = dict(ref.named_parameters()), dict(ref2.named_parameters())
    for n, p in task.named_parameters():
        mine, yard = rel_err(p.grad, rp[n].grad), rel_err(ap[n].grad, rp[n].grad)
        assert mine < 1.5 * yard + 1e-2, (n, mine, yard)


def _steps(task, opt, batch, n):
    losses = []
    for it in range(n):
        out = task.training_step(batch, it)
        opt.zero_grad(set_to_none=True)
        out['loss'].backward()
        opt.step()
        losses.append(float(out['loss']))
    torch.cuda.synchronize()
    return losses


def _state(task):
    return {k: v.detach().clone() for k, v in task.state_dict().items() if not k.startswith('input_tensors')}


def test_two_runs_are_bit_identical_vit_s_b64():
    g = torch.Generator().manual_seed(11)
    batch = {'image': torch.randn(64, 3, 224, 224, generator=g).cuda(), 'target': torch.randint(0, 10, (64,), generator=g).cuda()}
    results = []
    for _ in range(2):
        task, _ = _task_and_ref('vit_small_patch16_224', dict(img_size=224, drop_path_rate=0.1), 'AdamW', seed=9)
        task.cuda().train()
        opt = task.configure_optimizers()[0]['optimizer']
        torch.manual_seed(123)
        results.append((_steps(task, opt, batch, 2), _state(task)))
    assert results[0][0] == results[1][0]
    for k in results[0][1]:
        assert torch.equal(results[0][1][k], results[1][1][k]), k


def test_hipgraph_replay_equals_eager():
    from torchok_amd.engine.graph import GraphedTrainingStep
    g = torch.Generator().manual_seed(11)
    batch = {'image': torch.randn(16, 3, 224, 224, generator=g).cuda(), 'target': torch.randint(0, 6, (16,), generator=g).cuda()}
    results = []
    for graphed in (False, True):
        task, _ = _task_and_ref('vit_tiny_patch16_224', dict(img_size=224, depth=4), 'SGD', seed=9, classes=6)
        task.cuda().train()
        opt = task.configure_optimizers()[0]['optimizer']
        if graphed:
            step = GraphedTrainingStep(task, opt, batch, warmup=3)
            for _ in range(2):
                loss = float(step(batch)['loss'])
        else:
            loss = _steps(task, opt, batch, 5)[-1]
        torch.cuda.synchronize()
        results.append((loss, _state(task)))
    assert results[0][0] == results[1][0]
    for k in results[0][1]:
        assert torch.equal(results[0][1][k], results[1][1][k]), k
