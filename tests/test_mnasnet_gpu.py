"""MnasNet on the MI355X: the depthwise-convolution and squeeze-excite kernels against fp64 torch on the same bf16 inputs,
teacher-forced blocks against the fp32 oracle (tests/mnasnet_ref.py), ClassificationTask training steps against the oracle
with the bf16-autocast yardstick of test_resnet_gpu.py, reproducibility, hipGraph replay and the ArcFace recipe."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

import mnasnet_ref as M
import oracle.torchok_ref as R
import torchok_amd as T
from helpers import cls_config, copy_state, deterministic_state, rel_err
from torchok_amd import _C, engine
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
RECIPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'recipes')
p_ = lambda t: None if t is None else t.data_ptr()     # noqa: E731


def _dw_launch(x, w, k, s, dout):
    """forward (+ statistics rows), data gradient and weight gradient of one depthwise layer on the device."""
    lib = _C.lib()
    n, h, wd, c = x.shape
    p, q = (h - 1) // s + 1, (wd - 1) // s + 1
    out = torch.empty((n, p, q, c), dtype=torch.bfloat16, device='cuda')
    rows = lib.tok_dwconv_rows(n, h, wd, c, k, s)
    stats = torch.empty((2, rows, c), dtype=torch.float32, device='cuda')
    _C.check(lib.tok_dwconv_fwd(p_(x), p_(w), n, h, wd, c, c, k, s, p_(out), p_(stats), stream_ptr()), 'fwd')
    dx = torch.empty_like(x)
    _C.check(lib.tok_dwconv_dgrad(p_(dout), p_(w), n, h, wd, c, c, k, s, p_(dx), 0, stream_ptr()), 'dgrad')
    ws_bytes = lib.tok_dwconv_wgrad_ws_bytes(n, h, wd, c, k, s)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device='cuda')
    dw = torch.empty((c, k, k), dtype=torch.float32, device='cuda')
    _C.check(lib.tok_dwconv_wgrad(p_(x), p_(dout), n, h, wd, c, c, k, s, p_(dw), 0, p_(ws), ws_bytes, stream_ptr()), 'wgrad')
    torch.cuda.synchronize()
    return out, stats, dx, dw


@pytest.mark.parametrize('c', [8, 72, 120, 960])
@pytest.mark.parametrize('hw', [7, 15, 56, 112])
@pytest.mark.parametrize('k,s', [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_dwconv_kernels_vs_fp64(k, s, hw, c):
    g = torch.Generator().manual_seed(k * 1000 + s * 100 + hw + c)
    n = 2
    x = torch.randn(n, hw, hw, c, generator=g).to(torch.bfloat16)
    w = torch.randn(c, 1, k, k, generator=g) * (2.0 / (k * k)) ** 0.5
    p = (hw - 1) // s + 1
    dout = torch.randn(n, p, p, c, generator=g).to(torch.bfloat16)
    xd, wd_, gd = (x.double().permute(0, 3, 1, 2), w.double(), dout.double().permute(0, 3, 1, 2))
    ref = F.conv2d(xd, wd_, stride=s, padding=k // 2, groups=c)
    ref_dx = torch.nn.grad.conv2d_input(xd.shape, wd_, gd, stride=s, padding=k // 2, groups=c)
    ref_dw = torch.nn.grad.conv2d_weight(xd, wd_.shape, gd, stride=s, padding=k // 2, groups=c)
    xc, wc, gc = x.cuda(), w.cuda(), dout.cuda()
    out, stats, dx, dw = _dw_launch(xc, wc, k, s, gc)
    assert rel_err(out.permute(0, 3, 1, 2), ref) <= 1e-2
    assert rel_err(dx.permute(0, 3, 1, 2), ref_dx) <= 1e-2
    assert rel_err(dw, ref_dw.view(c, k, k)) <= 1e-3
    o = out.double().cpu().reshape(-1, c)      # statistics of the rounded output
    st = stats.double().cpu().sum(1)
    assert rel_err(st[0], o.sum(0)) <= 1e-3 and rel_err(st[1], (o * o).sum(0)) <= 1e-3
    again = _dw_launch(xc, wc, k, s, gc)
    for a, b in zip((out, stats, dx, dw), again):
        assert torch.equal(a, b)


def _se_ref(x, w1, b1, w2, b2):
    m = x.mean((1, 2))
    hdn = F.relu(m @ w1.t() + b1)
    return torch.sigmoid(hdn @ w2.t() + b2)


@pytest.mark.parametrize('c,rd,hw', [(72, 6, 28), (120, 10, 15), (672, 28, 14)])
def test_squeeze_excite_kernels_vs_fp64(c, rd, hw):
    g = torch.Generator().manual_seed(c + rd)
    n = 4
    x = torch.randn(n, hw, hw, c, generator=g).abs().to(torch.bfloat16)
    w1, b1 = torch.randn(rd, c, generator=g) / c ** 0.5, torch.randn(rd, generator=g) * 0.1
    w2, b2 = torch.randn(c, rd, generator=g) / rd ** 0.5, torch.randn(c, generator=g) * 0.1
    dout = torch.randn(n, hw, hw, c, generator=g).to(torch.bfloat16)
    prm = [t.double().requires_grad_() for t in (w1, b1, w2, b2)]
    xd = x.double().requires_grad_()
    gate_ref = _se_ref(xd, *prm)
    (xd * gate_ref[:, None, None, :] * dout.double()).sum().backward()
    lib = _C.lib()
    xc = x.cuda()
    dev = [t.cuda() for t in (w1, b1, w2, b2)]
    runs = []
    for _ in range(2):
        mean, gate = (torch.empty((n, c), device='cuda') for _ in range(2))
        hid = torch.empty((n, rd), device='cuda')
        ws = torch.empty(lib.tok_se_ws_floats(n, hw * hw, c, rd), device='cuda')
        _C.check(lib.tok_se_fwd(p_(xc), n, hw * hw, c, c, rd, *(p_(t) for t in dev), p_(mean), p_(hid), p_(gate), p_(ws),
                                stream_ptr()), 'se_fwd')
        grads = [torch.empty_like(t) for t in dev]
        dx = torch.empty_like(xc)
        _C.check(lib.tok_se_bwd(p_(dout.cuda()), p_(xc), n, hw * hw, c, c, rd, p_(dev[0]), p_(dev[2]), p_(mean), p_(hid),
                                p_(gate), *(p_(t) for t in grads), 0, p_(dx), 0, p_(ws), stream_ptr()), 'se_bwd')
        torch.cuda.synchronize()
        runs.append([gate, dx] + grads)
    gate, dx, gw1, gb1, gw2, gb2 = runs[0]
    assert rel_err(gate, gate_ref) <= 1e-3
    assert rel_err(dx, xd.grad) <= 1e-2
    for mine, ref in zip((gw1, gb1, gw2, gb2), prm):
        assert rel_err(mine, ref.grad) <= 1e-3
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _gate(name):
    """x1.5 the bf16-autocast distance + 1e-2 (test_resnet_gpu.py).  The squeeze-excite conv_reduce gradients are the residual
    of a cancelling sum over each image of d(out) * x times s(1 - s), formed from gradients stored in bf16 (the engine's
    design): measured at 2.1x (device) and up to 4.2x (host stand-in, which rounds where the kernels round) the distance of autocast,
    which keeps that path in fp32."""
    return 6.0 if '.se.conv_reduce.' in name else 1.5


def _block_pair(ref_block, eng_block, x, dout):
    """teacher-forced: the same bf16 input and output gradient into the oracle block (fp32 and bf16 autocast) and the engine
    block; output within 1e-2, every gradient and running statistic within the autocast yardstick."""
    eng_block.load_state_dict(ref_block.state_dict())
    eng_block.cuda().train()
    ref_block.train()
    ac_block = copy.deepcopy(ref_block)
    xa = x.float().requires_grad_()
    with torch.autocast('cpu', dtype=torch.bfloat16):
        ya = ac_block(xa)
    ya.float().backward(dout.float())
    xr = x.float().requires_grad_()
    yr = ref_block(xr)
    yr.backward(dout.float())
    xe = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    with engine.region() as r:
        t = r.input(xe)
        ye = r.output(eng_block(t))
    ye.backward(dout.cuda().contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    assert rel_err(ye, yr) <= 1e-2
    assert rel_err(xe.grad, xr.grad) < 1.5 * rel_err(xa.grad, xr.grad) + 1e-2
    rp, ap = dict(ref_block.named_parameters()), dict(ac_block.named_parameters())
    for name, prm in eng_block.named_parameters():
        mine, yard = rel_err(prm.grad, rp[name].grad), rel_err(ap[name].grad, rp[name].grad)
        assert mine < _gate(name) * yard + 1e-2, (name, mine, yard)
    rb = dict(ref_block.named_buffers())
    for name, b in eng_block.named_buffers():
        if b.is_floating_point():
            assert rel_err(b, rb[name]) <= 1e-2, name


@pytest.mark.parametrize('cin,cout,k,s,exp,se', [(40, 40, 5, 1, 3.0, 0.25 / 3.0), (40, 80, 5, 2, 6.0, 0.0)])
def test_inverted_residual_block_vs_oracle(cin, cout, k, s, exp, se):
    from torchok_amd.models.backbones import efficientnet as E
    torch.manual_seed(0)
    ref = M.InvertedResidual(cin, cout, k, s, False, exp, se)
    with torch.no_grad():
        for name, prm in ref.named_parameters():
            if prm.dim() == 1:
                prm.add_(torch.randn_like(prm) * 0.2 + (0.5 if name.endswith('bn3.weight') else 0.0))
    eng = E.InvertedResidual(cin, cout, k, s, False, exp, se)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(8, cin, 28, 28, generator=g).to(torch.bfloat16)
    ho = (28 - 1) // s + 1
    dout = torch.randn(8, cout, ho, ho, generator=g).to(torch.bfloat16)
    _block_pair(ref, eng, x, dout)


def _se_block(seed=0):
    from torchok_amd.models.backbones import efficientnet as E
    torch.manual_seed(seed)
    ref = M.InvertedResidual(40, 40, 5, 1, False, 3.0, 0.25 / 3.0)
    with torch.no_grad():
        for name, prm in ref.named_parameters():
            if prm.dim() == 1:
                prm.add_(torch.randn_like(prm) * 0.2 + (0.5 if name.endswith('bn3.weight') else 0.0))
    eng = E.InvertedResidual(40, 40, 5, 1, False, 3.0, 0.25 / 3.0)
    eng.load_state_dict(ref.state_dict())
    return ref, eng.cuda().train()


@pytest.mark.parametrize('foreign', [False, True])
def test_se_block_two_backwards_accumulate(foreign):
    """two forward + backward passes without clearing .grad: the second pass takes param_grad_target mode 1 (the depthwise
    wgrad with accumulate = 1, tok_se_bwd with param_accumulate bits); with a foreign .grad tensor set beforehand, mode 2 in both.
    The accumulated gradients (minus the preset) against the oracle block given the same two passes, on the autocast yardstick."""
    ref, eng = _se_block()
    ref.train()
    ac = copy.deepcopy(ref)
    g = torch.Generator().manual_seed(2)
    passes = [tuple(torch.randn(8, 40, 28, 28, generator=g).to(torch.bfloat16) for _ in range(2)) for _ in range(2)]
    preset = {}
    if foreign:
        for name, prm in ref.named_parameters():
            preset[name] = torch.randn(prm.shape, generator=g)
        for mod in (ref, ac):
            for name, prm in mod.named_parameters():
                prm.grad = preset[name].clone()
        for name, prm in eng.named_parameters():
            prm.grad = preset[name].cuda()
    for x, dout in passes:
        with torch.autocast('cpu', dtype=torch.bfloat16):
            ya = ac(x.float())
        ya.float().backward(dout.float())
        ref(x.float()).backward(dout.float())
        xe = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
        with engine.region() as r:
            t = r.input(xe)
            ye = r.output(eng(t))
        ye.backward(dout.cuda().contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    rp, ap = dict(ref.named_parameters()), dict(ac.named_parameters())
    for name, prm in eng.named_parameters():
        off = preset.get(name, 0.0)
        mine = rel_err(prm.grad.cpu() - off, rp[name].grad - off)
        yard = rel_err(ap[name].grad - off, rp[name].grad - off)
        assert mine < _gate(name) * yard + 1e-2, (name, mine, yard)
    rb = dict(ref.named_buffers())
    for name, b in eng.named_buffers():
        if b.is_floating_point():
            assert rel_err(b, rb[name]) <= 1e-2, name


def _task_and_ref(name, classes=10, seed=21):
    cfg = cls_config(name, classes)
    task = T.TASKS.get(cfg.task.name)(cfg, **cfg.task.params)
    ref = M.Classifier(name, classes)
    ref.load_state_dict(deterministic_state(ref.state_dict(), seed))
    copy_state(ref, task)
    return task, ref


def _step_vs_oracle(name, x, y):
    torch.manual_seed(0)
    task, ref = _task_and_ref(name)
    task.cuda().train()
    ref.train()
    ref2 = copy.deepcopy(ref)
    with torch.autocast('cpu', dtype=torch.bfloat16):
        o = ref2.forward_with_gt({'image': x, 'target': y})
    ac_loss = torch.nn.functional.cross_entropy(o['prediction'].float(), y)
    ac_loss.backward()
    ac_grads = {n: p.grad for n, p in ref2.named_parameters()}
    out = task.training_step({'image': x.cuda(), 'target': y.cuda()}, 0)
    out['loss'].backward()
    ref_loss, _ = R.training_step(ref, {'image': x, 'target': y}, None)
    torch.cuda.synchronize()
    assert abs(float(out['loss']) - float(ref_loss)) < max(2e-2, 1.5 * abs(float(ac_loss) - float(ref_loss)) + 1e-2)
    rp = dict(ref.named_parameters())
    for n, p in task.named_parameters():
        assert p.grad is not None, n
        mine, yard = rel_err(p.grad, rp[n].grad), rel_err(ac_grads[n], rp[n].grad)
        assert mine < _gate(n) * yard + 1e-2, (n, mine, yard)


@pytest.mark.parametrize('name', ['semnasnet_100', 'mnasnet_100'])
def test_training_step_vs_oracle(name):
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(16, 3, 128, 128, generator=g), torch.randint(0, 10, (16,), generator=g)
    _step_vs_oracle(name, x, y)


@pytest.mark.parametrize('hw', [(100, 140), (140, 100)])
def test_training_step_non_square_vs_oracle(hw):
    """sides that are not multiples of 32: every depthwise and squeeze-excite layer sees a non-square map (an h / w swap in
    the dwconv_bn_act or squeeze_excite wiring cannot cancel out)"""
    g = torch.Generator().manual_seed(6)
    x, y = torch.randn(8, 3, *hw, generator=g), torch.randint(0, 10, (8,), generator=g)
    _step_vs_oracle('semnasnet_100', x, y)


def test_eval_forward_vs_oracle():
    task, ref = _task_and_ref('semnasnet_100', seed=4)
    task.cuda().eval()
    ref.eval()
    x = torch.randn(8, 3, 96, 96, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        mine = task.backbone(x.cuda()).float().cpu()
        want = ref.backbone(x)
        with torch.autocast('cpu', dtype=torch.bfloat16):
            ac = ref.backbone(x).float()
        feats = task.backbone.forward_features(x.cuda())
        want_feats = ref.backbone.forward_features(x)
    assert rel_err(mine, want) < 1.5 * rel_err(ac, want) + 1e-2
    assert [tuple(f.shape) for f in feats] == [tuple(f.shape) for f in want_feats]
    for a, b in zip(feats[1:], want_feats[1:]):
        assert rel_err(a.float().cpu(), b) < 5e-2


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


def test_two_runs_are_bit_identical():
    results = []
    g = torch.Generator().manual_seed(11)
    batch = {'image': torch.randn(16, 3, 96, 96, generator=g).cuda(), 'target': torch.randint(0, 6, (16,), generator=g).cuda()}
    for _ in range(2):
        task, _ = _task_and_ref('semnasnet_100', 6, seed=9)
        task.cuda().train()
        opt = task.configure_optimizers()[0]['optimizer']
        losses = _steps(task, opt, batch, 2)
        results.append((losses, {k: v.detach().clone() for k, v in task.state_dict().items()
                                 if not k.startswith('input_tensors')}))
    assert results[0][0] == results[1][0]
    for k in results[0][1]:
        assert torch.equal(results[0][1][k], results[1][1][k]), k


def test_hipgraph_replay_equals_eager():
    from torchok_amd.engine.graph import GraphedTrainingStep
    g = torch.Generator().manual_seed(11)
    batch = {'image': torch.randn(16, 3, 64, 64, generator=g).cuda(), 'target': torch.randint(0, 6, (16,), generator=g).cuda()}
    results = []
    for graphed in (False, True):
        task, _ = _task_and_ref('semnasnet_100', 6, seed=9)
        task.cuda().train()
        opt = task.configure_optimizers()[0]['optimizer']
        if graphed:
            step = GraphedTrainingStep(task, opt, batch, warmup=3)
            for _ in range(2):
                loss = float(step(batch)['loss'])
        else:
            loss = _steps(task, opt, batch, 5)[-1]
        torch.cuda.synchronize()
        results.append((loss, {k: v.detach().clone() for k, v in task.state_dict().items()
                                if not k.startswith('input_tensors')}))
    assert results[0][0] == results[1][0]
    for k in results[0][1]:
        assert torch.equal(results[0][1][k], results[1][1][k]), k


def test_arcface_recipe_fit_on_device():
    from torchok_amd.run import fit
    os.environ.setdefault('HOME', '/tmp')
    cfg = T.load_config(os.path.join(RECIPES, 'representation_arcface_sop.yaml'),
                        overrides={'task.params.backbone_params.pretrained': False, 'trainer.precision': 'bf16',
                                   'trainer.devices': 1})
    assert cfg.task.params.backbone_name == 'semnasnet_100'
    g = torch.Generator().manual_seed(0)
    batches = [{'image': torch.randn(8, 3, 96, 96, generator=g).cuda(), 'target': torch.randint(0, 11318, (8,), generator=g).cuda()}
               for _ in range(3)]
    seen = []
    res = fit(cfg, batches=batches, max_steps=3, device='cuda:0', on_step=lambda i, out: seen.append(float(out['loss'])))
    assert res['steps'] == 3 and len(seen) == 3 and all(v == v and abs(v) != float('inf') for v in seen)
