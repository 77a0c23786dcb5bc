"""The launches of the conv units, pinned call for call on the host stand-in.

Every tok_* call the engine makes while a fixed list of cases runs forward and backward is logged as its name, its integer and
float arguments verbatim, the fields of a convolution descriptor, and `is None` for every pointer (no addresses).  So
tok_next_launch_event(*) arms the completion event and tok_next_launch_event(-) disarms it (_show).  A refusal is logged
as its exception type and message.  The log is compared with tests/golden/conv_unit_launch_trace.json, which was written by
`PYTHONPATH=. python tests/test_conv_unit_trace.py --write-golden` at the commit BEFORE the BatchNorm stage moved to engine/bn_stage.py (the
parent of the commit that added this file): host code above the C ABI may be rearranged, the launches may not change.

The cases reach every form of the BatchNorm stage (plain, plain + column sums, deferred, hard-swish, ReLU6, row-scaled, the stem
with its fused max-pool in both domains of its backward sums) and every rider of a data gradient (BN_SUMS on tok_conv_dgrad_bnstats
/ tok_conv_dgrad2 / tok_conv_dgrad_subacc, MASKED_DZ on tok_conv_dgrad_maskstore), each crossed with what requires a gradient
(the GRADS rows of test_bn_stage.py) and with BatchNorm in training mode, in eval mode and with track_running_stats=False.
2 x 8 x 8 inputs of 8-16 channels, except: the stem (3 -> 8 channels, 2 x 16 x 16) and the strided projection and one
fused bottleneck, which read maps of 64 channels because the stand-in's tok_conv_dgrad_subacc_ok and tok_conv_dgrad2_ok serve
c % 64 == 0 only.
The side-stream fork needs a device, so the `side` cases force it: paramgrad.goes_side answers True and Region.raw_event /
Region.fork_side are replaced by host versions that make the same two library calls."""
import contextlib
import ctypes
import json
import os
import sys

import pytest
import torch
import torch.nn as nn

import fake_backend as fb
from test_bn_stage import GRADS
from test_efficientnet_lite import LiteFake
from test_mobilenetv3 import V3Fake
from test_resnet_droppath import DropPathFake
from torchok_amd import _C
from torchok_amd.engine import functional as EF
from torchok_amd.engine import neck as EN
from torchok_amd.engine import paramgrad as PG
from torchok_amd.engine import resample as ER
from torchok_amd.engine.core import Region

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_unit_launch_trace.json')
BF = torch.bfloat16


class TraceFake(DropPathFake, V3Fake, LiteFake):
    """Every stand-in a conv unit can reach: grouped conv, phase moves and the row-scaled trio; depthwise conv and hard-swish; ReLU6."""


class Logged:
    """The stand-in behind a log of the calls the ENGINE makes (what a stand-in calls on itself is not a launch)."""

    def __init__(self, fake):
        self._fake, self.log = fake, []

    def __getattr__(self, name):
        fn = getattr(self._fake, name)
        if not name.startswith('tok_') or name == 'tok_last_error':
            return fn
        kinds = _C.PROTOTYPES[name][1]

        def call(*args):
            assert len(args) == len(kinds), name
            self.log.append([name] + [_entry(k, a) for k, a in zip(kinds, args)])
            return fn(*args)
        return call


def _entry(kind, a):
    if kind is ctypes.c_void_p:
        return a is None
    if kind is _C._PD:
        d = fb._desc(a)
        return {f: int(getattr(d, f)) for f, _ in _C.ConvDesc._fields_}
    if kind is ctypes.c_float:
        return float(a)
    assert isinstance(a, int) and not isinstance(a, bool), (kind, a)
    return a


# ---- the cases: name -> (knobs on engine.functional, builder); a builder returns (convs, bns, input shapes, forward) --------------

def _img(shape, seed, grad):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g).to(BF)
    if len(shape) == 4:
        t = t.contiguous(memory_format=torch.channels_last)
    return t.requires_grad_(grad)


def _conv_case(k, bias=False, bn=True, shortcut=False, defer=False, **kw):
    def build():
        conv = nn.Conv2d(8, 16, k, padding=k // 2, bias=bias)
        norm = nn.BatchNorm2d(16) if bn else None

        def forward(r, xs):
            extra = dict(kw, shortcut=xs[1]) if shortcut else dict(kw)
            if 'row_scale' in extra:
                extra['row_scale'] = torch.tensor([0.0, 2.0])            # one dropped, one kept sample (keep = 0.5)
            out = EF.conv_bn_act(r, xs[0], conv, norm, defer_apply=defer, **extra)
            return ER.fuse_sum_relu(r, [(out, 0)]) if defer else out       # (a deferred apply cannot leave the region)
        return [conv], [norm] if bn else [], [(2, 8, 8, 8)] + [(2, 16, 8, 8)] * shortcut, forward
    return build


def _linear():
    fc = nn.Linear(16, 10)
    return [fc], [], [(2, 16)], lambda r, xs: EF.linear(r, xs[0], fc)


def _stem():
    conv, bn = nn.Conv2d(3, 8, 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(8)
    return [conv], [bn], [(2, 3, 16, 16)], lambda r, xs: EF.conv_bn_act(r, xs[0], conv, bn, relu=True, pool=True)


def _bottleneck(c=8):
    """1x1 -> 3x3 (leaves column sums for) -> 1x1 + shortcut + ReLU (the fused unit 3 where it is served) -> a further 1x1"""
    convs = [nn.Conv2d(2 * c, c, 1, bias=False), nn.Conv2d(c, c, 3, padding=1, bias=False), nn.Conv2d(c, 2 * c, 1, bias=False),
             nn.Conv2d(2 * c, c, 1, bias=False)]
    bns = [nn.BatchNorm2d(c), nn.BatchNorm2d(c), nn.BatchNorm2d(2 * c), nn.BatchNorm2d(c)]

    def forward(r, xs):
        t = EF.conv_bn_act(r, xs[0], convs[0], bns[0], relu=True)
        t = EF.conv_bn_act(r, t, convs[1], bns[1], relu=True)
        t = EF.conv_bn_act(r, t, convs[2], bns[2], relu=True, shortcut=xs[0])
        return EF.conv_bn_act(r, t, convs[3], bns[3], relu=True)
    return convs, bns, [(2, 2 * c, 8, 8)], forward


def _strided_projection():
    """A residual unit (fused or not: its BatchNorm sums or its masked gradient ride), then a downsampling bottleneck: the stride-2
    projection runs on the subsampled input and parks its data gradient for conv1's"""
    convs = [nn.Conv2d(8, 64, 1, bias=False), nn.Conv2d(64, 8, 1, bias=False), nn.Conv2d(8, 8, 3, stride=2, padding=1, bias=False),
             nn.Conv2d(64, 16, 1, stride=2, bias=False), nn.Conv2d(8, 16, 1, bias=False)]
    bns = [nn.BatchNorm2d(64), nn.BatchNorm2d(8), nn.BatchNorm2d(8), nn.BatchNorm2d(16), nn.BatchNorm2d(16)]

    def forward(r, xs):
        x = EF.conv_bn_act(r, xs[0], convs[0], bns[0], relu=True, shortcut=xs[1])
        t = EF.conv_bn_act(r, x, convs[1], bns[1], relu=True)
        t = EF.conv_bn_act(r, t, convs[2], bns[2], relu=True)
        sc = EF.conv_bn_act(r, x, convs[3], bns[3])
        return EF.conv_bn_act(r, t, convs[4], bns[4], relu=True, shortcut=sc)
    return convs, bns, [(2, 8, 8, 8), (2, 64, 8, 8)], forward


def _phased():
    convs = [nn.Conv2d(8, 16, 1, bias=False), nn.Conv2d(16, 16, 3, padding=2, dilation=2, bias=False)]
    bns = [nn.BatchNorm2d(16), nn.BatchNorm2d(16)]

    def forward(r, xs):
        t = EF.phase_split(r, xs[0], 2)
        t = EF.conv_bn_act(r, t, convs[0], bns[0], relu=True)
        return EF.from_phase(r, EF.conv_bn_act(r, t, convs[1], bns[1], relu=True))
    return convs, bns, [(2, 8, 8, 8)], forward


def _depthwise():
    conv, bn = nn.Conv2d(16, 16, 3, padding=1, groups=16, bias=False), nn.BatchNorm2d(16)
    return [conv], [bn], [(2, 16, 8, 8)], lambda r, xs: EF.dwconv_bn_act(r, xs[0], conv, bn, relu=True)


def _grouped():
    conv, bn = nn.Conv2d(16, 16, 3, padding=1, groups=4, bias=False), nn.BatchNorm2d(16)
    return [conv], [bn], [(2, 16, 8, 8)], lambda r, xs: EF.conv_bn_act(r, xs[0], conv, bn, relu=True)


def _neck():
    conv, bn = nn.Conv2d(24, 16, 1, bias=False), nn.BatchNorm2d(16)
    return [conv], [bn], [(2, 8, 8, 8), (2, 16, 4, 4)], lambda r, xs: EN.upsample_concat_conv_bn_relu(r, xs, (8, 8), conv, bn)


CASES = {}
for _k in (1, 3):
    CASES.update({
        f'conv{_k}_none': ({}, _conv_case(_k, relu=False)),
        f'conv{_k}_relu': ({}, _conv_case(_k, relu=True)),
        f'conv{_k}_relu_shortcut': ({}, _conv_case(_k, relu=True, shortcut=True)),
        f'conv{_k}_hard_swish': ({}, _conv_case(_k, act=EF.HARD_SWISH)),
        f'conv{_k}_relu6': ({}, _conv_case(_k, act=EF.RELU6)),
        f'conv{_k}_row_scale': ({}, _conv_case(_k, relu=True, shortcut=True, row_scale=True)),
        f'conv{_k}_defer_apply': ({}, _conv_case(_k, defer=True)),
        f'conv{_k}_bias_no_bn': ({}, _conv_case(_k, bias=True, bn=False)),
        # refused combinations
        f'conv{_k}_hard_swish_shortcut': ({}, _conv_case(_k, act=EF.HARD_SWISH, shortcut=True)),
        f'conv{_k}_relu_no_bn': ({}, _conv_case(_k, bn=False, relu=True)),
        f'conv{_k}_row_scale_pool': ({}, _conv_case(_k, relu=True, shortcut=True, row_scale=True, pool=True)),
    })
CASES.update({
    'linear': ({}, _linear),
    'stem_pooled_stats': ({'STEM_POOLED_STATS': True}, _stem),
    'stem_position_stats': ({'STEM_POOLED_STATS': False}, _stem),
    'bottleneck_fused': ({'UNIT3_MIN_ROWS': 0}, _bottleneck),
    'bottleneck_fused_c64': ({'UNIT3_MIN_ROWS': 0}, lambda: _bottleneck(64)),     # (tok_conv_dgrad2_ok)
    'bottleneck_plain': ({'UNIT3_MIN_ROWS': 1 << 40}, _bottleneck),
    'strided_projection': ({'SUBSAMPLE_MIN_ROWS': 0, 'UNIT3_MIN_ROWS': 1 << 40}, _strided_projection),
    'strided_projection_fused': ({'SUBSAMPLE_MIN_ROWS': 0, 'UNIT3_MIN_ROWS': 0}, _strided_projection),
    'phased': ({}, _phased),
    'depthwise_k3': ({}, _depthwise),
    'grouped_w4': ({}, _grouped),
    'commuted_neck': ({}, _neck),
})


def _bn_train(bn):
    pass


def _bn_eval(bn):
    bn.eval()


def _bn_untracked(bn):
    bn.track_running_stats = False


BN_MODES = {'train': _bn_train, 'eval': _bn_eval, 'untracked': _bn_untracked}
SIDE = 'side'      # (grads 'all', BatchNorm in training mode, every weight gradient forked behind its unit's apply launch)


def _keys():
    keys = []
    for case, (_, build) in CASES.items():
        modes = sorted(BN_MODES) if build()[1] else ['train']
        keys += [f'{case}/{grads}/{mode}' for grads in sorted(GRADS) for mode in modes]
        keys.append(f'{case}/all/{SIDE}')
    return keys


def _force_side(patch):
    lib = _C.lib()

    def raw_event(self):
        return lib.tok_event_create()

    def fork_side(self, keep_alive, raw_event=None):
        if raw_event is not None:
            _C.check(lib.tok_stream_wait_event(None, raw_event), 'tok_stream_wait_event')
        return contextlib.nullcontext()
    patch(PG, 'goes_side', lambda node, g, policy, rows=0: True)
    patch(Region, 'raw_event', raw_event)
    patch(Region, 'fork_side', fork_side)


def trace(key):
    """The log of one case.  Everything it patches is put back."""
    case, grads, mode = key.split('/')
    knobs, build = CASES[case]
    w, g, b, x, grad_mode = GRADS[grads]
    undo = []

    def patch(obj, name, value):
        undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)
    token = fb.install(TraceFake())
    logged = Logged(token[0])
    patch(_C, '_lib', logged)
    patch(PG, '_plans', {})         # (asked of the library once per layer shape: every case starts without the answers)
    try:
        for name, value in knobs.items():
            patch(EF, name, value)
        if mode == SIDE:
            _force_side(patch)
        torch.manual_seed(0)
        convs, bns, shapes, forward = build()
        for conv in convs:
            conv.weight.requires_grad_(w)
            if conv.bias is not None:
                conv.bias.requires_grad_(w)
        for bn in bns:
            bn.weight.requires_grad_(g)
            bn.bias.requires_grad_(b)
            BN_MODES.get(mode, _bn_train)(bn)
        xs = [_img(s, 3 + i, x and s[1] % 8 == 0) for i, s in enumerate(shapes)]
        try:
            with torch.set_grad_enabled(grad_mode):
                r = Region()
                ins = [r.input(t, c_pad_to=8 if t.shape[1] % 8 == 0 else 4) for t in xs]
                y = r.output(forward(r, ins))
            if y.requires_grad:
                logged.log.append(['backward'])
                y.backward(_img(tuple(y.shape), 77, False).to(y.dtype))
        except Exception as e:      # a refusal is part of the contract: its type and its text
            logged.log.append(['raised', type(e).__name__, str(e)])
    finally:
        for obj, name, value in reversed(undo):
            setattr(obj, name, value)
        fb.uninstall(token)
    return logged.log


def _show(call):
    """A logged call as the golden file spells it: name(args), `*` a pointer that was given, `-` one that was None, a convolution
    descriptor as {n;h;w;c;k;r;s;p;q;stride;pad;s_pad}; the two markers as plain words."""
    if call[0] in ('backward', 'raised'):
        return ' '.join(call)
    args = ['*-'[a] if isinstance(a, bool) else '{%s}' % ';'.join(str(v) for v in a.values()) if isinstance(a, dict) else repr(a)
            for a in call[1:]]
    return f"{call[0]}({','.join(args)})"


def write_golden():
    """Run at the commit the launches are pinned FROM (see the module docstring), never to make a failing test pass.  Every
    distinct call and every distinct run is stored once: calls[i] a string (_show), runs[j] indices into calls,
    cases[case]['grads/mode'] = j."""
    calls, runs, cases = {}, {}, {}
    for key in _keys():
        run = tuple(calls.setdefault(_show(c), len(calls)) for c in trace(key))
        cases.setdefault(key.split('/')[0], {})[key.split('/', 1)[1]] = runs.setdefault(run, len(runs))
    with open(GOLDEN, 'w') as f:
        f.write('{"calls": [\n%s\n],\n"runs": [\n%s\n],\n"cases": {\n%s\n}}\n' % (
            ',\n'.join(json.dumps(c) for c in calls), ',\n'.join(json.dumps(r, separators=(',', ':')) for r in runs),
            ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in cases.items())))


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        doc = json.load(f)
    return {f'{case}/{rest}': [doc['calls'][i] for i in doc['runs'][j]] for case, v in doc['cases'].items() for rest, j in v.items()}


def test_the_case_list_is_the_golden_files(golden):
    assert sorted(golden) == sorted(_keys())


@pytest.mark.parametrize('key', _keys())
def test_launches_are_those_of_the_parent(golden, key):
    got, want = [_show(c) for c in trace(key)], golden[key]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f'{key}: call {i} is {a}, the parent made {b}'
    assert len(got) == len(want), f'{key}: {len(got)} calls, the parent made {len(want)}: {got[len(want):] or want[len(got):]}'


def test_the_cases_reach_every_form_and_every_rider(golden):
    """(of the golden file itself: a case list that lost a form would pin nothing about it)"""
    seen = {c.split('(')[0] for calls in golden.values() for c in calls}
    for name in ('tok_bn_act_fwd', 'tok_bn_act_fwd_colsum', 'tok_bn_bwd_reduce', 'tok_bn_bwd_apply', 'tok_bn_eval_coeffs',
                 'tok_bn_hswish_fwd', 'tok_bn_hswish_bwd_reduce', 'tok_bn_hswish_bwd_apply',
                 'tok_bn_relu6_fwd', 'tok_bn_relu6_bwd_reduce', 'tok_bn_relu6_bwd_apply',
                 'tok_bn_droppath_fwd', 'tok_bn_droppath_bwd_reduce', 'tok_bn_droppath_bwd_apply',
                 'tok_bn_relu_maxpool_fwd', 'tok_bn_pool_bwd_reduce_pooled', 'tok_bn_pool_bwd_reduce', 'tok_bn_pool_bwd_apply',
                 'tok_fuse_sum_affine_relu_fwd', 'tok_conv_fwd_bn_apply', 'tok_bn_gram_finalize', 'tok_bn3_bwd_prepare',
                 'tok_conv_dgrad', 'tok_conv_dgrad_bnstats', 'tok_conv_dgrad_maskstore', 'tok_conv_dgrad2', 'tok_conv_dgrad_subacc',
                 'tok_subsample2_fwd', 'tok_phase_split', 'tok_dwconv_fwd', 'tok_gconv_fwd', 'tok_bilinear_sum_stats',
                 'tok_next_launch_event', 'tok_stream_wait_event'):
        assert name in seen, name
    # BN_SUMS and MASKED_DZ on the sub-accumulating data gradient: bn_y given / mask_store set
    subacc = [c[:-1].split(',') for calls in golden.values() for c in calls if c.startswith('tok_conv_dgrad_subacc(')]
    assert any(a[5] == '*' for a in subacc) and any(a[8] == '1' for a in subacc)
    events = [c for c in golden[f'conv3_relu_shortcut/all/{SIDE}'] if c.startswith('tok_next_launch_event')]
    assert events == ['tok_next_launch_event(*)', 'tok_next_launch_event(-)']      # armed, disarmed


if __name__ == '__main__':
    if sys.argv[1:] != ['--write-golden']:
        sys.exit('usage: PYTHONPATH=. python tests/test_conv_unit_trace.py --write-golden   (at the commit the launches are pinned from)')
    write_golden()
