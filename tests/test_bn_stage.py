"""The BatchNorm stage every "producer -> BatchNorm -> activation" unit shares (engine/functional.py: batch_stats, bn_coeffs,
bn_apply, _ConvBnActNode._bn_bwd), pinned per unit on the host stand-in: the refusals of the depthwise unit and of the neck
(only the conv unit's tests pinned them before), when tok_bn_act_fwd is handed a ReLU mask pointer and when tok_bn_finalize is
handed the running statistics.  The mask rules differ between the units and are pinned as they are:
  conv_bn_act:  ReLU and gradients on (whatever requires a gradient);
  dwconv_bn_act: ReLU, gradients on, and the filter, the input, BatchNorm's weight or BatchNorm's bias requires a gradient;
  commuted neck: ReLU, gradients on, and the filter, a source or BatchNorm's weight (not its bias) requires a gradient."""
import pytest
import torch
import torch.nn as nn

import fake_backend as fb
from test_mobilenetv3 import V3Fake
from torchok_amd.engine import functional as EF
from torchok_amd.engine import neck as EN
from torchok_amd.engine.core import Region

EVAL_AFFINE = 'gradients of BatchNorm affine parameters in eval mode'
MOMENTUM_NONE = r'BatchNorm momentum=None \(cumulative average\)'


class StageFake(V3Fake):
    """Keeps, per call, which of the pointers this file asks about were given."""

    def __init__(self):
        super().__init__()
        self.masks, self.tracked, self.eval_coeffs = [], [], 0

    def tok_bn_act_fwd(self, y, scale, shift, shortcut, relu, out, mask, m, c, st):
        self.masks.append(mask is not None)
        return super().tok_bn_act_fwd(y, scale, shift, shortcut, relu, out, mask, m, c, st)

    def tok_bn_eval_coeffs(self, *args):
        self.eval_coeffs += 1
        return super().tok_bn_eval_coeffs(*args)

    def tok_bn_finalize(self, stats, rows, count, cp, c, gamma, beta, rm, rv, nbt, *rest):
        assert (rm is None) == (rv is None) == (nbt is None)
        self.tracked.append(rm is not None)
        return super().tok_bn_finalize(stats, rows, count, cp, c, gamma, beta, rm, rv, nbt, *rest)


@pytest.fixture
def fake():
    token = fb.install(StageFake())
    yield token[0]
    fb.uninstall(token)


def _bf(shape, seed, grad):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(grad)


def _conv(k):
    def make(hw=8):
        conv, bn = nn.Conv2d(8, 16, k, padding=k // 2, bias=False), nn.BatchNorm2d(16)
        return conv, bn, [(2, 8, hw, hw)], lambda r, xs, **kw: EF.conv_bn_act(r, xs[0], conv, bn, **kw)
    return make


def _depthwise(hw=8, c=16):
    conv, bn = nn.Conv2d(c, c, 3, padding=1, groups=c, bias=False), nn.BatchNorm2d(c)
    return conv, bn, [(2, c, hw, hw)], lambda r, xs, **kw: EF.dwconv_bn_act(r, xs[0], conv, bn, **kw)


def _neck(hw=8):
    conv, bn = nn.Conv2d(24, 16, 1, bias=False), nn.BatchNorm2d(16)
    return conv, bn, [(2, 8, hw, hw), (2, 16, hw // 2, hw // 2)], \
        lambda r, xs, **kw: EN.upsample_concat_conv_bn_relu(r, xs, (hw, hw), conv, bn, **kw)


UNITS = {'conv1x1': _conv(1), 'conv3x3': _conv(3), 'depthwise_k3': _depthwise, 'commuted_neck': _neck}
ACTS = {'none': dict(relu=False), 'relu': dict(relu=True), 'hard_swish': dict(relu=False, act=EF.HARD_SWISH)}
# what requires a gradient: (filter, BatchNorm weight, BatchNorm bias, input), and whether gradients are on at all
GRADS = {'all': (True, True, True, True, True), 'nothing': (False, False, False, False, True),
         'bn_weight_only': (False, True, False, False, True), 'bn_bias_only': (False, False, True, False, True),
         'input_only': (False, False, False, True, True), 'no_grad': (True, True, True, True, False)}
UNIT_ACTS = [(u, a) for u in sorted(UNITS) for a in sorted(ACTS) if (u, a) != ('commuted_neck', 'hard_swish')]   # (no such neck)


def _mask_expected(unit, relu, w, g, b, x, grad_mode):
    """The parent's rule of each unit (module docstring)."""
    if unit.startswith('conv'):
        return relu and grad_mode
    if unit == 'depthwise_k3':
        return relu and grad_mode and (w or x or g or b)
    return relu and grad_mode and (w or x or g)


def _run(fake, unit, act_kw, grads, bn_setup=None):
    w, g, b, x, grad_mode = grads
    torch.manual_seed(0)
    conv, bn, shapes, forward = UNITS[unit]()
    conv.weight.requires_grad_(w)
    bn.weight.requires_grad_(g)
    bn.bias.requires_grad_(b)
    if bn_setup is not None:
        bn_setup(bn)
    xs = [_bf(s, 3 + i, x) for i, s in enumerate(shapes)]
    with torch.set_grad_enabled(grad_mode):
        r = Region()
        out = forward(r, [r.input(t) for t in xs], **act_kw)
        r.output(out)
    return bn


@pytest.mark.parametrize('grads', sorted(GRADS))
@pytest.mark.parametrize('unit,act', UNIT_ACTS)
def test_relu_mask_pointer_follows_each_units_rule(fake, unit, act, grads):
    _run(fake, unit, ACTS[act], GRADS[grads])
    if unit == 'commuted_neck':
        assert 'bilinear_sum_stats' in fake.calls
    if act == 'hard_swish':
        assert fake.masks == [] and fake.calls.count('bn_hswish_fwd') == 1      # the mask-less path: no tok_bn_act_fwd at all
    else:
        assert fake.masks == [bool(_mask_expected(unit, act == 'relu', *GRADS[grads]))]


def _train_tracking(bn):
    pass


def _train_not_tracking(bn):       # FreezeUnfreeze: train mode, the running buffers kept but not updated
    bn.track_running_stats = False


def _train_no_buffers(bn):         # built with track_running_stats=False: there are no running buffers
    bn.track_running_stats = False
    bn.running_mean = bn.running_var = bn.num_batches_tracked = None


def _eval_no_buffers(bn):          # eval mode without running statistics still normalises with the batch's
    _train_no_buffers(bn)
    bn.eval()


@pytest.mark.parametrize('setup', [_train_tracking, _train_not_tracking, _train_no_buffers, _eval_no_buffers],
                         ids=lambda f: f.__name__[1:])
@pytest.mark.parametrize('unit,act', UNIT_ACTS)
def test_finalize_gets_running_statistics_only_when_they_are_tracked(fake, unit, act, setup):
    bn = _run(fake, unit, ACTS[act], GRADS['all'], setup)
    assert fake.tracked == [bool(bn.training and bn.track_running_stats)]
    if setup is _train_tracking:
        assert fake.tracked == [True] and int(bn.num_batches_tracked) == 1
    elif bn.running_mean is not None:
        assert int(bn.num_batches_tracked) == 0 and bool((bn.running_mean == 0).all())


@pytest.mark.parametrize('unit', sorted(UNITS))
def test_eval_mode_takes_the_running_statistics_and_no_finalize(fake, unit):
    """(the neck leaves the commuted order for the direct one: bilinear concat, then the conv unit)"""
    _run(fake, unit, ACTS['relu'], GRADS['input_only'], lambda bn: bn.eval())
    assert fake.tracked == [] and fake.eval_coeffs == 1
    assert 'bilinear_sum_stats' not in fake.calls


def _backward_error(fake, unit, hw, c=None):
    torch.manual_seed(0)
    conv, bn, shapes, forward = UNITS[unit](hw) if c is None else UNITS[unit](hw, c)
    bn.eval()
    r = Region()
    y = r.output(forward(r, [r.input(_bf(s, 5, True)) for s in shapes], relu=True))
    with pytest.raises(NotImplementedError, match=EVAL_AFFINE) as e:
        y.backward(torch.ones_like(y))
    return e.value


def test_depthwise_unit_refuses_affine_gradients_in_eval_mode_like_the_conv_unit(fake):
    dw = _backward_error(fake, 'depthwise_k3', 6, 8)
    cv = _backward_error(fake, 'conv3x3', 6)
    assert type(dw) is type(cv) is NotImplementedError and str(dw) == str(cv) == EVAL_AFFINE


@pytest.mark.parametrize('unit', sorted(UNITS))
def test_momentum_none_is_refused_in_forward(fake, unit):
    """Cumulative-average BatchNorm is not built.  The neck falls to the direct order (it never starts its own launches) and is
    refused there, by the conv unit."""
    def setup(bn):
        bn.momentum = None
    with pytest.raises(NotImplementedError, match=MOMENTUM_NONE):
        _run(fake, unit, ACTS['relu'], GRADS['all'], setup)
    assert fake.tracked == [] and fake.masks == []
    if unit == 'commuted_neck':
        assert 'bilinear_sum_stats' not in fake.calls and 'conv_fwd' in fake.calls
