"""Fused units recorded on the engine tape.  Each function launches the forward kernels through
the C ABI and (in grad mode) appends a Node whose ``backward`` launches the backward kernels.

Unit                      replaces (reference / [timm] / ATen)
------------------------  -------------------------------------------------------------------
conv_bn_act               conv2d -> batch_norm -> (+ shortcut) -> relu   ([timm] Bottleneck /
                          BasicBlock / downsample_conv; resnet.py:488-490; convbnact.py:48-53)
max_pool_3x3_s2           nn.MaxPool2d(3, 2, 1)                          (resnet.py:510)
global_avg_pool           SelectAdaptivePool2d('avg', flatten=True)      (pooling.py:7-12)
linear                    nn.Linear                                      (linear_head.py:31)
dwconv_bn_act             depthwise conv -> batch_norm -> relu           ([timm] DepthwiseSeparableConv / InvertedResidual)
gconv_bn_act              grouped 3x3 conv -> batch_norm -> relu         ([timm] Bottleneck.conv2 with groups = cardinality: ResNeXt)
squeeze_excite            x * gate(expand(relu(reduce(mean(x)))))        ([timm] efficientnet_blocks.SqueezeExcite;
                          gate = sigmoid or hard sigmoid)
phase_split / phase_merge the layout a dilated ResNet stage runs in: conv2d(dilation=d, padding=d) as the plain 3x3 on the d x d
                          phase images (resnet.py:363-405 with output_stride 8 / 16)

conv_bn_act / dwconv_bn_act take act='hard_swish' (MobileNetV3) or act='relu6' (EfficientNet-Lite): the mask-less activation
path of csrc/bn.hip.
"""
import weakref
from typing import Optional, Tuple

import os

import torch
from torch import nn

from .. import _C
from .core import _ms as _core_ms
from . import paramgrad as PG
from .core import (BF16, Node, Region, TTensor, await_ready, donate_grad, grad_target, is_last_contribution, pad8, ptr,
                   refuse_phased, stream_ptr)

F32 = torch.float32


# ---- packed bf16 operands of the fp32 master weights ------------------------------------------------

class _Packs:
    """bf16 MFMA operands derived from one fp32 master weight: the forward pack [Kp][R][Sp][Cp]
    and the dgrad pack [Cp][R][S][Kp] (flipped taps).  Re-derived whenever `refresh` is asked
    (every training forward: the optimizer has moved the master since)."""
    __slots__ = ('fwd', 'dgrad', 'bias', 'key', 'synced', 'dims')

    def __init__(self):
        self.fwd = None
        self.dgrad = None
        self.bias = None
        self.key = None
        self.synced = None   # weight._version the packs were derived at (None: unknown / stale)
        self.dims = None     # (k, r, s, c, kp, sp, cp)


_packs = {}  # id(weight) -> (weakref(weight), _Packs); Tensor.__eq__ rules out a WeakKeyDictionary


def _packs_for(weight) -> _Packs:
    ent = _packs.get(id(weight))
    if ent is not None and ent[0]() is weight:
        return ent[1]
    pk = _Packs()
    key = id(weight)
    _packs[key] = (weakref.ref(weight, lambda _r, key=key: _packs.pop(key, None)), pk)
    return pk


def _krsc(weight: torch.Tensor):
    """(K, R, S, C) of a conv (K,C,R,S) or linear (K,C) master and a guarantee that its
    physical layout is [k][r][s][c]."""
    if weight.dim() == 2:
        if not weight.is_contiguous():
            raise RuntimeError('linear weight must be contiguous')
        return weight.shape[0], 1, 1, weight.shape[1]
    k, c, r, s = weight.shape
    if not weight.permute(0, 2, 3, 1).is_contiguous():
        # re-home the master in channels-last order once (logical shape / state_dict unchanged)
        weight.data = weight.data.contiguous(memory_format=torch.channels_last)
        if not weight.permute(0, 2, 3, 1).is_contiguous():  # degenerate dims: force strides
            weight.data = torch.as_strided(weight.data.permute(0, 2, 3, 1).contiguous().view(-1),
                                           (k, c, r, s), (r * s * c, 1, s * c, c))
    return k, r, s, c


def get_packs(weight: nn.Parameter, bias: Optional[nn.Parameter], kp: int, sp: int, cp: int,
              want_dgrad: bool, refresh: bool) -> _Packs:
    pk = _packs_for(weight)
    k, r, s, c = _krsc(weight)
    key = (weight.data_ptr(), kp, sp, cp, weight.device)
    lib = _C.lib()
    st = stream_ptr()
    global _pack_generation
    # packs stay valid while the master is untouched: torch-visible writes bump `_version`; the fused
    # optimizers (whose kernels do not) refresh every pack themselves right after the step (repack_after_step)
    stale = pk.key != key or (refresh and pk.synced != weight._version)
    if want_dgrad and (pk.fwd is None or pk.dgrad is None or stale):
        if pk.fwd is None or pk.key != key:
            pk.fwd = torch.empty((kp, r, sp, cp), dtype=BF16, device=weight.device)
            _pack_generation += 1
        if pk.dgrad is None or pk.key != key:
            pk.dgrad = torch.empty((cp, r, s, kp), dtype=BF16, device=weight.device)
            _pack_generation += 1
        _C.check(lib.tok_pack_weight_both(ptr(weight), k, r, s, c, ptr(pk.fwd), kp, sp, cp, ptr(pk.dgrad), st),
                 'tok_pack_weight_both')
        pk.synced = weight._version
    elif pk.fwd is None or stale:
        if pk.fwd is None or pk.key != key:
            pk.fwd = torch.empty((kp, r, sp, cp), dtype=BF16, device=weight.device)
            _pack_generation += 1
        if pk.key != key:
            pk.dgrad = None
        _C.check(lib.tok_pack_weight_fwd(ptr(weight), k, r, s, c, ptr(pk.fwd), kp, sp, cp, st),
                 'tok_pack_weight_fwd')
        if pk.dgrad is not None:       # an older dgrad pack is no longer in step with the master
            pk.dgrad = None
            _pack_generation += 1
        pk.synced = weight._version
    pk.dims = (k, r, s, c, kp, sp, cp)
    if bias is not None:
        if kp == k:
            pk.bias = bias.detach()
        else:
            if pk.bias is None or pk.bias.shape[0] != kp:
                pk.bias = torch.zeros(kp, dtype=F32, device=weight.device)
            pk.bias[:k] = bias.detach()
    else:
        pk.bias = None
    pk.key = key
    return pk


WGRAD_SIDE_STREAM = os.environ.get('TOK_WGRAD_SIDE', '1') == '1'
# which weight gradients go to the side stream: the LDS/MFMA-bound ones (filters larger than 1x1), whose resource profile
# complements the HBM-bound main chain, and the short-M or MFMA-bound pointwise ones (_wgrad_side_ok).  Measured (ResNet-50,
# unit-3 fusion on): every weight gradient on the side stream 21.58, this choice 21.45 ms/step
WGRAD_SIDE_MAX_ROWS = int(os.environ.get('TOK_WGRAD_SIDE_MAX_ROWS', '100000'))
# long-M pointwise weight gradients stay on the main stream when they are HBM-bound like the chain they would fight (ResNet-50: 51-102
# MACs per operand element), and go to the side stream when they are MFMA-bound (HRNet-W48's 720 -> 720 neck convolution over 786 432
# pixels: 360): HRNet-W48 70.65 -> 69.83 ms/step, ResNet-50 / SwinV2-T unchanged (profiles/r05_side_stream_resweep.txt)
WGRAD_SIDE_MIN_INTENSITY = float(os.environ.get('TOK_WGRAD_SIDE_MIN_INTENSITY', '128'))


def _wgrad_side_ok(r, s, m, k, c) -> bool:
    return r * s > 1 or m < WGRAD_SIDE_MAX_ROWS or (k * c) / float(k + c) >= WGRAD_SIDE_MIN_INTENSITY


# Only units of the MAIN stream fork their weight gradients to the side stream (round 6).  A unit recorded on a branch stream
# (HRNet's low-resolution branches, SwinV2's position-bias chain) keeps them on its own stream: with three branch streams + the
# side stream there are more streams than hardware queues (two share one), and the side queue — every weight gradient of every
# branch in one FIFO — was 33 ms busy beside a 46-ms HRNet-W48 backward.  HRNet-W48 B=24: 67.1 -> 66.1 ms/step (nobody forks:
# 66.1 as well; only the branches fork: 67.9).


def _side_for_tag(tag, region=None) -> bool:
    # ... and nobody forks in a region whose main stream and branch streams alone fill the four hardware queues (HRNet-W48: main +
    # three branches; a fifth stream shares a queue with one of them: 65.4 vs 65.9 ms/step without the side stream, same box)
    if tag:
        return False
    return region is None or len(getattr(region, '_streams', ())) < 3


_pack_generation = 0   # bumped whenever a pack buffer is (re)allocated: invalidates cached batch tables


def invalidate_packs():
    """Force every bf16 operand pack to be re-derived at its next use.  Needed only after writing a weight
    behind torch's back (`p.data.mul_(...)`, a custom kernel): such writes do not bump `p._version`."""
    for _, pk in list(_packs.values()):
        pk.synced = None


def repack_after_step(params, cache: dict, arena_sig) -> None:
    """Refresh the packs of every weight in `params` with ONE launch (tok_pack_weights_batched).  Called by
    the fused optimizers at the end of step(): their kernels update the masters without touching
    `_version`, so this is what keeps packs and masters in step."""
    import ctypes
    sig = (_pack_generation, arena_sig)
    if cache.get('sig') != sig:
        items, entries, skipped = [], [], []
        block = 0
        for p in params:
            ent = _packs.get(id(p))
            if ent is None or ent[0]() is not p:
                continue
            pk = ent[1]
            if pk.fwd is None or pk.key is None or pk.dims is None or pk.key[0] != p.data_ptr():
                skipped.append(pk)
                continue
            k, r, s, c, kp, sp, cp = pk.dims
            it = _C.PackItem(p.data_ptr(), pk.fwd.data_ptr(), pk.dgrad.data_ptr() if pk.dgrad is not None else None,
                             k, r, s, c, kp, sp, cp, block)
            nb = _C.lib().tok_pack_item_blocks(ctypes.byref(it))
            if nb <= 0:                       # a pack of 2^31 elements or more: refreshed on its own by the forward
                skipped.append(pk)
                continue
            block += nb
            items.append(it)
            entries.append((p, pk))
        dev = None
        if items:
            arr = (_C.PackItem * len(items))(*items)
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
            dev = host.to(entries[0][0].device)
        cache.clear()
        cache.update(sig=sig, dev=dev, n=len(items), blocks=block, entries=entries, skipped=skipped)
    for pk in cache['skipped']:
        pk.synced = None
    if cache['n']:
        _C.check(_C.lib().tok_pack_weights_batched(ptr(cache['dev']), cache['n'], cache['blocks'], stream_ptr()),
                 'tok_pack_weights_batched')
        for p, pk in cache['entries']:
            pk.synced = p._version


def _conv_desc(x: TTensor, k_pad: int, r: int, s: int, stride: int, pad: int) -> _C.ConvDesc:
    if x.data.dim() == 2:      # (N, Cp) rows: the 1x1 / h = w = 1 case (Linear)
        n, cp = x.shape
        h = w = 1
    else:
        n, h, w, cp = x.shape
    p = (h + 2 * pad - r) // stride + 1
    q = (w + 2 * pad - s) // stride + 1
    return _C.ConvDesc(n, h, w, cp, k_pad, r, s, p, q, stride, pad, 8 if cp == 4 else s)


def _phased_conv_ok(conv: nn.Module, phase: int) -> bool:
    """Does this layer commute with the phase layout of its input?  A 1x1 / stride-1 convolution does; a 3x3 / stride-1 one
    whose dilation and padding both equal the phase IS the plain padding-1 convolution on every phase image."""
    if not isinstance(conv, nn.Conv2d) or isinstance(conv.padding, str):
        return False
    ks, st, pd, dl = tuple(conv.kernel_size), tuple(conv.stride), tuple(conv.padding), tuple(conv.dilation)
    if ks == (1, 1):
        return st == (1, 1) and pd == (0, 0) and dl == (1, 1)
    return ks == (3, 3) and st == (1, 1) and dl == (phase, phase) and pd == (phase, phase)


def _check_conv(conv: nn.Conv2d, phase: int = 1):
    """`phase` != 1: the caller has checked the layer with _phased_conv_ok (its dilation is then the phase, and served)."""
    if conv.groups != 1 or (phase == 1 and tuple(conv.dilation) != (1, 1)):
        raise NotImplementedError('torchok_amd conv: dilation == 1 and groups == 1 (dense, conv_bn_act), groups == channels '
                                  '(depthwise 3x3 / 5x5, dwconv_bn_act) or a grouped 3x3 of group width 4, 8, 16, 32 or 64 '
                                  '(gconv_bn_act) only')
    if conv.kernel_size[0] != conv.kernel_size[1] or conv.stride[0] != conv.stride[1] \
            or conv.padding[0] != conv.padding[1] or isinstance(conv.padding, str):
        raise NotImplementedError('torchok_amd conv: square kernel / stride / padding only')
    if conv.padding_mode != 'zeros':
        raise NotImplementedError('torchok_amd conv: zero padding only')


# ---- conv + bn + (add) + relu ------------------------------------------------------------------------

RELU = 'relu'
HARD_SWISH = 'hard_swish'
RELU6 = 'relu6'
# the mask-less activations -> the entry-point family tok_bn_<family>_fwd / _bwd_reduce / _bwd_apply that serves them
MASKLESS = {HARD_SWISH: 'hswish', RELU6: 'relu6'}


def _check_act(relu, act, bn, shortcut=None, pool=False, defer_apply=False):
    """The unit's one activation, None / RELU / HARD_SWISH / RELU6, from the public keywords.  act=None: what `relu` says.
    act='hard_swish' or 'relu6' (`relu` is not looked at): BatchNorm + that activation on tok_bn_hswish_* / tok_bn_relu6_*,
    which keep no mask and know no shortcut, pooled or deferred form (MobileNetV3 and EfficientNet-Lite never activate after
    a residual add)."""
    if act is None:
        return RELU if relu else None
    if act not in MASKLESS:
        raise NotImplementedError(f'torchok_amd activation {act!r}: None (ReLU / identity by `relu`), {HARD_SWISH!r} or {RELU6!r}')
    if bn is None or shortcut is not None or pool or defer_apply:
        raise NotImplementedError(f"act={act!r}: BatchNorm units without shortcut, pool or defer_apply only")
    return act


def _maskless(lib, act, stage):
    """(entry point, its name) of a mask-less activation's `stage`: 'fwd', 'bwd_reduce' or 'bwd_apply'."""
    name = f'tok_bn_{MASKLESS[act]}_{stage}'
    return getattr(lib, name), name


# ---- the BatchNorm stage of a unit: every "producer -> BatchNorm -> activation" unit takes it from here ---------------

def batch_stats(bn: nn.BatchNorm2d) -> bool:
    """Does this BatchNorm normalise with the statistics of the batch (training mode, or no running statistics kept)?"""
    return bn.training or bn.running_mean is None


def bn_coeffs(lib, st, bn, stats, rows, m, kp, dev):
    """(scale, shift, mean, rstd) per channel: from the producer's partial sums `stats` [2][rows][kp] over m rows (running
    statistics updated when the module tracks them), or, stats=None, from the running statistics (mean = rstd = None)."""
    # one allocation for the per-channel vectors (an allocator call costs the launch thread 2-3 us; HRNet-W48 makes 307
    # of these units per step)
    vec = torch.empty((4, kp), dtype=F32, device=dev)
    scale, shift = vec[0], vec[1]
    if stats is None:
        _C.check(lib.tok_bn_eval_coeffs(ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var),
                                        float(bn.eps), kp, bn.num_features, ptr(scale), ptr(shift), st), 'tok_bn_eval_coeffs')
        return scale, shift, None, None
    if bn.momentum is None:
        raise NotImplementedError('BatchNorm momentum=None (cumulative average)')
    mean, rstd = vec[2], vec[3]
    track = bn.training and bn.track_running_stats and bn.running_mean is not None
    _C.check(lib.tok_bn_finalize(ptr(stats), rows, m, kp, bn.num_features, ptr(bn.weight), ptr(bn.bias),
                                 ptr(bn.running_mean) if track else None, ptr(bn.running_var) if track else None,
                                 ptr(bn.num_batches_tracked) if track else None, float(bn.momentum), float(bn.eps),
                                 ptr(mean), ptr(rstd), ptr(scale), ptr(shift), st), 'tok_bn_finalize')
    return scale, shift, mean, rstd


def bn_apply(lib, st, y, scale, shift, act, shortcut, want_mask, m, kp, row_scale=None):
    """The plain apply pass out = act(y * scale + shift (+ shortcut)) -> (out_data, mask).  `want_mask` is the caller's
    rule for keeping the ReLU bits; hard-swish and ReLU6 keep none.
    row_scale (stochastic depth, a ReLU unit with a shortcut): out = relu(s[sample] * (y * scale + shift) + shortcut), the sample
    of a row being row // (m // len(row_scale))."""
    out_data = torch.empty_like(y)
    if act in MASKLESS:
        fwd, name = _maskless(lib, act, 'fwd')
        _C.check(fwd(ptr(y), ptr(scale), ptr(shift), ptr(out_data), m, kp, st), name)
        return out_data, None
    mask = torch.empty((m, kp // 8), dtype=torch.uint8, device=y.device) if want_mask else None
    if row_scale is not None:
        _C.check(lib.tok_bn_droppath_fwd(ptr(y), ptr(scale), ptr(shift), ptr(shortcut.data), ptr(row_scale),
                                         m // row_scale.numel(), ptr(out_data), ptr(mask), m, kp, st), 'tok_bn_droppath_fwd')
        return out_data, mask
    _C.check(lib.tok_bn_act_fwd(ptr(y), ptr(scale), ptr(shift), ptr(shortcut.data) if shortcut is not None else None,
                                int(act == RELU), ptr(out_data), ptr(mask), m, kp, st), 'tok_bn_act_fwd')
    return out_data, mask


class _ConvBnActNode(Node):
    needs_backward = True
    act = None                      # None / RELU / HARD_SWISH / RELU6 (the last two: dz is recomputed from y, no mask)
    relu = property(lambda self: self.act == RELU)

    def __init__(self):
        self.x = self.out = self.shortcut = None
        self.y = self.mask = None
        self.region = None
        self.fused_partial = None   # (partial, rows) when a consumer's dgrad epilogue did our BN-bwd reduce
        self.pool = None            # tap indices of the fused 3x3/s2 max-pool: `out` is the POOLED map, z was never stored
        self.ypool = None           # raw conv output at the winning taps (pooled-domain BatchNorm-backward sums)
        self.row_scale = None       # per-sample fp32 factor of the BatchNorm output (stochastic depth): the tok_bn_droppath_* trio

    def release(self):
        self.x = self.out = self.shortcut = None
        self.y = self.pk = self.mask = self.fused_partial = self.pool = self.ypool = None
        self.mean = self.rstd = self.scale = self.shift = self.row_scale = None

    def wants_fused_bwd_stats(self) -> bool:
        """Can the kernel that completes d(out) also reduce sum(dz), sum(dz*y) for this unit?"""
        # (the dgrad epilogues know the ReLU mask only: a hard-swish or ReLU6 producer takes the stand-alone reduce, and so does
        # a unit with a row scale, whose dz is not mask * d(out))
        return (self.bn is not None and self.batch_stats and self.pool is None and self.row_scale is None
                and (self.act is None or (self.act == RELU and self.mask is not None)))

    def _apply_bwd(self, lib, st, g, mask, coef, dy, ds_ptr, ds_acc, m, kp):
        """dy = c1*dz + c2*y + c3 (and the shortcut's dz) for the unit's activation."""
        if self.act in MASKLESS:
            bwd_apply, name = _maskless(lib, self.act, 'bwd_apply')
            _C.check(bwd_apply(ptr(g), ptr(self.y), ptr(self.scale), ptr(self.shift), ptr(coef), ptr(dy), m, kp, st), name)
        elif self.row_scale is not None:
            _C.check(lib.tok_bn_droppath_bwd_apply(ptr(g), ptr(self.y), ptr(mask), ptr(self.row_scale), m // self.row_scale.numel(),
                                                   ptr(coef), ptr(dy), ds_ptr, ds_acc, m, kp, st), 'tok_bn_droppath_bwd_apply')
        else:
            _C.check(lib.tok_bn_bwd_apply(ptr(g), ptr(self.y), ptr(mask), ptr(self.scale), ptr(self.shift), ptr(coef),
                                          int(self.relu), ptr(dy), ds_ptr, ds_acc, m, kp, st), 'tok_bn_bwd_apply')

    def _finalize_bwd(self, lib, st, g, mask, m, kp, g_need, b_need):
        """sum(dz), sum(dz*xhat) -> dgamma, dbeta; returns the apply coefficients (stand-alone reduce / finalize launches)."""
        bn = self.bn
        dzy = 0
        if self.fused_partial is not None:
            partial, rows = self.fused_partial   # reduced by the dgrad that completed d(out)
            dzy = 1
        else:
            rows = lib.tok_bn_bwd_rows(m, kp)
            if self.pool is not None and self.ypool is not None:
                # sums over the pooled elements (each feeds exactly one position): 3 pooled-size reads, no gather
                mp = self.out.data.numel() // kp
                rows = lib.tok_bn_bwd_rows(mp, kp)
                partial = torch.empty((2, rows, kp), dtype=F32, device=g.device)
                _C.check(lib.tok_bn_pool_bwd_reduce_pooled(ptr(g), ptr(self.out.data), ptr(self.ypool), ptr(self.mean),
                                                           ptr(self.rstd), mp, kp, ptr(partial), st),
                         'tok_bn_pool_bwd_reduce_pooled')
            elif self.pool is not None:
                partial = torch.empty((2, rows, kp), dtype=F32, device=g.device)
                n_, h_, w_, _ = self.y.shape
                _C.check(lib.tok_bn_pool_bwd_reduce(ptr(g), ptr(self.pool), ptr(self.y), ptr(self.scale), ptr(self.shift),
                                                    ptr(self.mean), ptr(self.rstd), n_, h_, w_, kp, ptr(partial), st),
                         'tok_bn_pool_bwd_reduce')
            elif self.act in MASKLESS:
                partial = torch.empty((2, rows, kp), dtype=F32, device=g.device)
                bwd_reduce, name = _maskless(lib, self.act, 'bwd_reduce')
                _C.check(bwd_reduce(ptr(g), ptr(self.y), ptr(self.scale), ptr(self.shift), ptr(self.mean), ptr(self.rstd), m, kp,
                                    ptr(partial), st), name)
            elif self.row_scale is not None:
                partial = torch.empty((2, rows, kp), dtype=F32, device=g.device)
                _C.check(lib.tok_bn_droppath_bwd_reduce(ptr(g), ptr(self.y), ptr(mask), ptr(self.row_scale),
                                                        m // self.row_scale.numel(), ptr(self.mean), ptr(self.rstd), m, kp,
                                                        ptr(partial), st), 'tok_bn_droppath_bwd_reduce')
            else:
                partial = torch.empty((2, rows, kp), dtype=F32, device=g.device)
                _C.check(lib.tok_bn_bwd_reduce(ptr(g), ptr(self.y), ptr(mask), ptr(self.scale), ptr(self.shift),
                                               ptr(self.mean), ptr(self.rstd), int(self.relu), m, kp, ptr(partial), st),
                         'tok_bn_bwd_reduce')
        coef = torch.empty((3, kp), dtype=F32, device=g.device)
        gbuf, bbuf, acc, finish = PG.pair_sinks(bn.weight if g_need else None, bn.bias if b_need else None)
        _C.check(lib.tok_bn_bwd_finalize(ptr(partial), rows, m, kp, bn.num_features, ptr(bn.weight), ptr(self.mean),
                                         ptr(self.rstd), ptr(gbuf), ptr(bbuf), ptr(coef), acc, dzy, st), 'tok_bn_bwd_finalize')
        finish()
        return coef

    def _bn_bwd(self, lib, st, g, m, kp, need_dy, apply=None):
        """The BatchNorm (+ activation) backward of the unit: dgamma / dbeta, then dy — None when nobody needs it.
        `apply(mask, coef, dy)` stands in for the plain apply launch (the conv unit's own forms)."""
        bn = self.bn
        g_need, b_need = bn.weight.requires_grad, bn.bias.requires_grad
        mask = self.mask if self.act == RELU else None
        if self.batch_stats:
            coef = self._finalize_bwd(lib, st, g, mask, m, kp, g_need, b_need)
        else:
            # eval-mode BN: y -> out is a fixed affine map: dy = scale * dz, dgamma/dbeta unsupported
            if g_need or b_need:
                raise NotImplementedError('gradients of BatchNorm affine parameters in eval mode')
            coef = torch.zeros((3, kp), dtype=F32, device=g.device)
            coef[0] = self.scale
        if not need_dy:
            return None
        dy = torch.empty_like(self.y)
        if apply is not None:
            apply(mask, coef, dy)
        else:
            self._apply_bwd(lib, st, g, mask, coef, dy, None, 0, m, kp)
        return dy

    def backward(self):
        lib, st = _C.lib(), stream_ptr()
        out: TTensor = self.out
        g = out.grad
        if g is None:
            return
        apply_event = None
        conv, bn, d = self.conv, self.bn, self.desc
        m, kp = self.y.numel() // self.y.shape[-1], self.y.shape[-1]
        x: TTensor = self.x
        w_need = conv.weight.requires_grad
        x_need = x.requires_grad
        bias_need = conv.bias is not None and conv.bias.requires_grad
        sc: Optional[TTensor] = self.shortcut
        # decided ONCE: the BatchNorm apply launch carries the completion event iff the weight gradient forks behind it
        side = w_need and PG.goes_side(self, g, PG.CONV, m)

        if bn is not None:
            sc_need = sc is not None and sc.requires_grad

            def apply(mask, coef, dy):
                nonlocal apply_event
                if side and self.pool is None and self.act not in MASKLESS:
                    # the weight gradient will be forked to the side stream behind THIS apply pass: the pass carries the
                    # completion event itself (no event-record packet on the main queue)
                    apply_event = self.region.raw_event()     # armed right in front of the launch that carries it (below)
                ds_ptr, ds_acc = None, 0
                if sc_need:
                    if sc.grad is None and out.grad_owned:
                        # in-place mask of the incoming gradient, then donate it to the shortcut
                        ds_ptr = ptr(g)
                        donate_grad(sc, g)
                    else:
                        tgt, ds_acc = grad_target(sc)
                        ds_ptr = ptr(tgt)
                if self.pool is not None:
                    n_, h_, w_, _ = self.y.shape
                    _C.check(lib.tok_bn_pool_bwd_apply(ptr(g), ptr(self.pool), ptr(self.y), ptr(self.scale), ptr(self.shift),
                                                       ptr(coef), n_, h_, w_, kp, ptr(dy), st), 'tok_bn_pool_bwd_apply')
                    return
                if apply_event is not None:
                    lib.tok_next_launch_event(apply_event)
                try:
                    self._apply_bwd(lib, st, g, mask, coef, dy, ds_ptr, ds_acc, m, kp)
                finally:
                    if apply_event is not None:
                        lib.tok_next_launch_event(None)   # never left armed for an unrelated later launch
            dy = self._bn_bwd(lib, st, g, m, kp, w_need or x_need or bias_need or sc_need, apply)
        else:
            dy = g  # plain conv (+bias): the output gradient IS dy
        out.grad = None
        if dy is None:
            return
        # the bias gradient (column sums of dy) rides the weight-gradient kernel where that serves the layer
        bias_in_wgrad = bool(bias_need and w_need and PG.wgrad_plan(d)[0])
        if bias_need and not bias_in_wgrad:
            bs, bacc = PG.sink(conv.bias)
            # tall dy (a conv / token GEMM bias): coalesced row-chunk partials, then a fixed-order fold
            PG.colsum(dy, m, kp, bs, bacc, two_pass=m > 4096 and kp == conv.bias.shape[0], n_real=conv.bias.shape[0])
            PG.commit(conv.bias, bs, bacc)
        # the weight gradient is started BEFORE its unit's data gradient (started after it: 22.0 vs 21.1 ms/step, the later
        # start costs more).  Nothing on the main chain waits for dW: the LDS/MFMA-bound (3x3) and short-M ones run on the side
        # stream beside the HBM-bound BatchNorm passes and the dgrad of the units below, joined at the end of the region; the
        # long-M pointwise ones are HBM-bound themselves and would only fight the chain for bandwidth (PG.CONV)
        if w_need:
            k, _, _, c = _krsc(conv.weight)
            PG.run_beside(self, side, (x.data, dy), raw_event=apply_event, fn=lambda: PG.weight_grad(
                d, x.data, dy, k, c, weight=conv.weight, bias=conv.bias if bias_in_wgrad else None)[1:])
        if x_need:
            prod = x.node
            rider = _dgrad_rider(x)
            sub = x.grad_sub if getattr(self, 'sub_capable', False) else None
            tgt, acc = grad_target(x, sub_ok=sub is not None)
            partial = _rider_partial(lib, rider, prod, d, x.cp, g.device)
            bn_y = ptr(prod.y) if rider == BN_SUMS else None
            bn_mask = ptr(prod.mask) if (rider == MASKED_DZ or (rider == BN_SUMS and prod.relu)) else None
            if sub is not None:
                # d(x) = this data gradient + the parked gradient of x[:, ::2, ::2] (a strided projection shortcut): one
                # launch, d(x) written once, with the rider's epilogue
                x.grad_sub = None
                assert acc == 0
                _C.check(lib.tok_conv_dgrad_subacc(d, ptr(dy), ptr(self.pk.dgrad), ptr(tgt), ptr(sub), bn_y, bn_mask, ptr(partial),
                                                   int(rider == MASKED_DZ), st), 'tok_conv_dgrad_subacc')
            elif rider == MASKED_DZ:
                _C.check(lib.tok_conv_dgrad_maskstore(d, ptr(dy), ptr(self.pk.dgrad), ptr(tgt), acc, bn_mask, ptr(partial), st),
                         'tok_conv_dgrad_maskstore')
            elif rider == BN_SUMS:
                _C.check(lib.tok_conv_dgrad_bnstats(d, ptr(dy), ptr(self.pk.dgrad), ptr(tgt), acc, bn_y, bn_mask, ptr(partial), st),
                         'tok_conv_dgrad_bnstats')
            else:
                _C.check(lib.tok_conv_dgrad(d, ptr(dy), ptr(self.pk.dgrad), ptr(tgt), acc, st), 'tok_conv_dgrad')


# ---- who rides a data gradient ------------------------------------------------------------------------------------------
# The launch that completes d(x) can finish work of the unit that produced x in its epilogue:
BN_SUMS = 'bn_sums'          # the BatchNorm-backward sums sum(dz), sum(dz * y) of a _ConvBnActNode (saves it a pass over d(x) and y)
MASKED_DZ = 'masked_dz'      # dz = relu_mask * d(out) and sum(dz) of a fused _Unit3Node (what its backward and its shortcut consume)


def _dgrad_rider(x: TTensor):
    """What rides the next data gradient into `x`: BN_SUMS, MASKED_DZ or None.  Only the last contribution completes d(x), and
    only once per producer."""
    prod = x.node
    if (isinstance(prod, _ConvBnActNode) and is_last_contribution(x) and prod.wants_fused_bwd_stats()
            and prod.fused_partial is None):
        return BN_SUMS
    # (a fused unit WITHOUT activation has no ReLU bits: its d(out) is dz itself and takes the plain path)
    if (isinstance(prod, _Unit3Node) and prod.relu and prod.mask is not None and is_last_contribution(x)
            and prod.masked_partial is None):
        return MASKED_DZ
    return None


def _rider_partial(lib, rider, prod, d, cp: int, dev) -> Optional[torch.Tensor]:
    """The (2, rows, cp) partial sums the data gradient of layer `d` writes for `rider`, left on the producer for its backward."""
    if rider is None:
        return None
    rows = lib.tok_conv_dgrad_stat_rows(d)
    partial = torch.empty((2, rows, cp), dtype=F32, device=dev)
    if rider == MASKED_DZ:
        prod.masked_partial = (partial, rows)
    else:
        prod.fused_partial = (partial, rows)
    return partial


# ---- unit 3 of a bottleneck: 1x1 conv -> BatchNorm -> + shortcut -> ReLU without the pre-normalisation tensor ----------

FUSE_UNIT3 = os.environ.get('TOK_FUSE_UNIT3', '1') != '0'
# the fused unit trades ~27 tensor-units of HBM traffic for a handful of small launches (Gram matrix, two K x P x P products):
# it pays where the 4P-channel maps are large (ResNet-50 at batch 256: layers 1-2 and, marginally, 3)
UNIT3_MIN_ROWS = int(os.environ.get('TOK_UNIT3_MIN_ROWS', '100000'))   # measured: 0 -> 22.4, 40000 -> 22.0, 100000 -> 21.8, plain 23.2 ms/step


def _pointwise_desc(x: TTensor, k: int) -> _C.ConvDesc:
    n, h, w, cp = x.shape
    return _C.ConvDesc(n, h, w, cp, k, 1, 1, h, w, 1, 0, 1)


def _colsum_f32(t: torch.Tensor, m: int, c: int) -> torch.Tensor:
    out = torch.empty(c, dtype=F32, device=t.device)
    PG.colsum(t, m, c, out, 0, two_pass=m > 4096, n_real=c)
    return out


class _Unit3Node(Node):
    """out = relu(bn(conv1x1(x)) + shortcut) with the BatchNorm statistics taken from the second moments of x and the whole
    backward written on x, dz = relu_mask * d(out) and small P x P / K x P matrices (csrc/unit3.hip).  The K-channel tensor
    between conv and BatchNorm (and its gradient) never exists."""
    needs_backward = True

    def __init__(self):
        self.x = self.out = self.shortcut = self.mask = None
        self.relu = True
        self.masked_partial = None      # (partial, rows): the launch that completed d(out) already stored dz and sum(dz)

    def release(self):
        self.x = self.out = self.shortcut = self.mask = self.masked_partial = None
        self.mean = self.rstd = self.wz = self.zsum = self.pk = None

    def backward(self):
        lib, st = _C.lib(), stream_ptr()
        out: TTensor = self.out
        g = out.grad
        if g is None:
            return
        conv, bn, d, x, sc = self.conv, self.bn, self.desc, self.x, self.shortcut
        kp, p = d.k, d.c
        m = d.n * d.p * d.q
        dev = g.device
        # 1. dz = relu_mask * d(out) (d(out) itself for a unit without activation) and the partial sums of dz
        if self.masked_partial is not None:
            partial, rows = self.masked_partial
            dz = g
        else:
            rows = lib.tok_bn_bwd_rows(m, kp)
            partial = torch.empty((2, rows, kp), dtype=F32, device=dev)
            dz = g if (out.grad_owned or not self.relu) else torch.empty_like(g)
            _C.check(lib.tok_relu_mask_reduce(ptr(g), ptr(self.mask) if self.relu else None, m, kp, ptr(dz), ptr(partial), st),
                     'tok_relu_mask_reduce')
        out.grad = None
        # 2. the shortcut receives dz itself; a projection shortcut of the same kind (conv1x1 + BatchNorm, no activation,
        #    nobody else reads its output) inherits the partial sums of dz as well
        if sc is not None and sc.requires_grad:
            if donate_grad(sc, dz):
                scn = sc.node
                if isinstance(scn, _Unit3Node) and not scn.relu and sc.uses == 1 and scn.masked_partial is None:
                    scn.masked_partial = (partial, rows)
            else:
                tgt, _ = grad_target(sc)
                tgt.add_(dz)
        w_need = conv.weight.requires_grad
        x_need = x.requires_grad
        g_need, b_need = bn.weight.requires_grad, bn.bias.requires_grad
        if not (w_need or x_need or g_need or b_need):
            return
        # 3. G = dz^T x   (the weight-gradient launch, on dz)
        G = PG.weight_grad(d, x.data, dz, kp, p)[0]
        # 4. dgamma / dbeta / dW, coefficients and the two operands of the data gradient
        gbuf, bbuf, pacc, finish = PG.pair_sinks(bn.weight if g_need else None, bn.bias if b_need else None)
        dw, wacc = PG.sink(conv.weight) if w_need else (torch.empty((kp, p), dtype=F32, device=dev), 0)
        coef = torch.empty((3, kp), dtype=F32, device=dev)
        wa = torch.empty((p, kp), dtype=BF16, device=dev)
        wb = torch.empty((p, p), dtype=BF16, device=dev)
        cvec = torch.empty(p, dtype=F32, device=dev)
        scratch = torch.empty(lib.tok_bn3_bwd_prepare_ws_floats(p, kp), dtype=F32, device=dev)
        _C.check(lib.tok_bn3_bwd_prepare(ptr(G), ptr(conv.weight), ptr(self.wz), ptr(self.zsum), ptr(partial), rows, m, p,
                                         kp, ptr(bn.weight), ptr(self.mean), ptr(self.rstd), ptr(gbuf), ptr(bbuf), pacc,
                                         ptr(coef), ptr(dw), wacc, ptr(wa), ptr(wb), ptr(cvec), ptr(scratch), st),
                 'tok_bn3_bwd_prepare')
        finish()
        if w_need:
            PG.commit(conv.weight, dw, wacc)
        if not x_need:
            return
        # 5. d(x) = dz wa + x wb + cvec  (+ the BatchNorm-backward sums of the unit that produced x)
        prod = x.node
        fuse = _dgrad_rider(x) == BN_SUMS        # (the masked-dz store is not an epilogue of these launches)
        tgt, acc = grad_target(x)
        dpp = _pointwise_desc(x, p)
        part2 = _rider_partial(lib, BN_SUMS if fuse else None, prod, dpp, p, dev)
        bn_y = ptr(prod.y) if fuse else None
        bn_mask = ptr(prod.mask) if (fuse and prod.relu) else None
        if lib.tok_conv_dgrad2_ok(d, dpp):
            # both products in one launch of the ring kernel: d(x) is stored once
            _C.check(lib.tok_conv_dgrad2(d, ptr(dz), ptr(wa), dpp, ptr(x.data), ptr(wb), ptr(cvec), ptr(tgt), acc, bn_y, bn_mask,
                                         ptr(part2), st), 'tok_conv_dgrad2')
        else:
            _C.check(lib.tok_conv_dgrad(d, ptr(dz), ptr(wa), ptr(tgt), acc, st), 'tok_conv_dgrad')
            _C.check(lib.tok_conv_dgrad_bias(dpp, ptr(x.data), ptr(wb), ptr(cvec), ptr(tgt), 1, bn_y, bn_mask, ptr(part2), st),
                     'tok_conv_dgrad_bias')
        if self.region is not None:
            self.region.keep_until_join(dz, wa, wb, cvec, G, scratch)


def _unit3_forward(region: Region, x: TTensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, shortcut: Optional[TTensor], kp: int,
                   relu: bool) -> TTensor:
    lib, st = _C.lib(), stream_ptr()
    dev = x.data.device
    if bn.momentum is None:
        raise NotImplementedError('BatchNorm momentum=None (cumulative average)')
    d = _pointwise_desc(x, kp)
    p = x.cp
    m = d.n * d.p * d.q
    pk = get_packs(conv.weight, None, kp, 1, p, want_dgrad=False, refresh=True)
    # batch statistics of conv(x) from the second moments of x:  Z = x^T x  and  colsum(x)
    dz_ = _pointwise_desc(x, p)
    zz = PG.weight_grad(dz_, x.data, x.data, p, p)[0]
    if x.colsum_part is not None:
        part, nrows = x.colsum_part        # left behind by the activation pass that produced x
        zsum = torch.empty(p, dtype=F32, device=x.data.device)
        _C.check(lib.tok_colsum_f32(ptr(part), nrows, p, ptr(zsum), 0, st), 'tok_colsum_f32')
        x.colsum_part = None
    else:
        zsum = _colsum_f32(x.data, m, p)
    mean, rstd, scale, shift = (torch.empty(kp, dtype=F32, device=dev) for _ in range(4))
    wz = torch.empty((kp, p), dtype=F32, device=dev)       # W Z: the statistics now, the weight gradient later
    track = bn.training and bn.track_running_stats and bn.running_mean is not None
    _C.check(lib.tok_bn_gram_finalize(ptr(zz), ptr(zsum), ptr(conv.weight), m, p, kp, ptr(bn.weight), ptr(bn.bias),
                                      ptr(bn.running_mean) if track else None, ptr(bn.running_var) if track else None,
                                      ptr(bn.num_batches_tracked) if track else None, float(bn.momentum), float(bn.eps),
                                      ptr(mean), ptr(rstd), ptr(scale), ptr(shift), ptr(wz), st), 'tok_bn_gram_finalize')
    out_data = torch.empty((d.n, d.p, d.q, kp), dtype=BF16, device=dev)
    training = region.grad_mode and (conv.weight.requires_grad or x.requires_grad or bn.weight.requires_grad
                                     or (shortcut is not None and shortcut.requires_grad))
    mask = torch.empty((m, kp // 8), dtype=torch.uint8, device=dev) if (training and relu) else None
    _C.check(lib.tok_conv_fwd_bn_apply(d, ptr(x.data), ptr(pk.fwd), ptr(scale), ptr(shift),
                                       ptr(shortcut.data) if shortcut is not None else None, int(relu), ptr(out_data),
                                       ptr(mask), st), 'tok_conv_fwd_bn_apply')
    out = TTensor(out_data, kp, requires_grad=bool(training))
    if training:
        node = _Unit3Node()
        node.x, node.out, node.shortcut, node.mask, node.relu = x, out, shortcut, mask, relu
        node.conv, node.bn, node.desc, node.pk = conv, bn, d, pk
        node.mean, node.rstd, node.wz, node.zsum = mean, rstd, wz, zsum
        out.node = node
        if x.requires_grad:
            x.uses += 1
        if shortcut is not None and shortcut.requires_grad:
            shortcut.uses += 1
        region.add(node)
    return out


def _inherit_phase(out: TTensor, x: TTensor) -> TTensor:
    """The output of a unit that ran on phase images is in the phase layout of its input."""
    if x.phase != 1:
        out.phase, out.phase_steps = x.phase, x.phase_steps
    return out


FUSE_STEM_POOL = os.environ.get('TOK_FUSE_STEM_POOL', '1') != '0'
STEM_POOLED_STATS = os.environ.get('TOK_STEM_POOLED_STATS', '1') != '0'   # BatchNorm-backward sums of the fused stem in the pooled domain


def conv_bn_act(region: Region, x: TTensor, conv: nn.Module, bn: Optional[nn.BatchNorm2d] = None,
                relu: bool = False, shortcut: Optional[TTensor] = None, pool: bool = False, defer_apply: bool = False,
                act: Optional[str] = None, row_scale: Optional[torch.Tensor] = None) -> TTensor:
    """out = act(bn(conv(x)) (+ shortcut)).  `conv` is an nn.Conv2d or nn.Linear used purely as
    the parameter container (state_dict names stay those of the reference).
    act=None: ReLU or no activation, as `relu` says.  act='hard_swish' / 'relu6' (BatchNorm, no shortcut / pool / defer_apply):
    the activation is hard-swish / ReLU6 and `relu` is not looked at; the unit keeps y and no mask, its backward recomputes z
    from y, it never becomes the fused unit 3 and its BatchNorm-backward sums are never taken by a consumer's data gradient.
    pool=True (BatchNorm + ReLU, no shortcut): out = maxpool3x3/s2/p1(act(bn(conv(x)))) with the activated map never
    stored (the ResNet stem when only the pooled map is consumed).
    defer_apply=True (BatchNorm, no activation, no shortcut — the last unit of an HRNet fuse path): the apply pass is NOT run;
    the returned tensor holds the RAW convolution output and carries `.affine = (scale, shift)` for a consumer that applies
    them itself (resample.fuse_sum_relu: the write and the read of the normalised term are one fma there).  Its backward is
    the unit's usual one (it never reads the normalised values of a unit without activation).
    An input in phase layout (phase_split; `bn=None` too): a 1x1 / stride-1 convolution on any phase, or a 3x3 / stride-1
    nn.Conv2d whose dilation == padding == (x.phase, x.phase), which runs as the padding-1 convolution on x.data (descriptor
    pad = 1; packs and every backward route are the plain ones).  The output inherits the phase; a shortcut must be in the same
    phase layout.  A dilation that is not the tensor's phase is refused as it always was; every other layer refuses a phased
    tensor through await_ready.
    row_scale (stochastic depth; BatchNorm + ReLU + shortcut on a 4-D input, no pool / defer_apply / act=): an fp32 vector with one
    factor per SAMPLE, 0 for a dropped sample and 1 / keep for a kept one: out = relu(row_scale[i] * bn(conv(x)) + shortcut) on the
    tok_bn_droppath_* trio (csrc/bn_droppath.hip).  BatchNorm sees the un-dropped convolution output, with batch or with
    running statistics.  The unit never becomes the fused unit 3 and never hands its BatchNorm-backward sums to a consumer's
    data gradient.  In phase layout the phase images of a sample are contiguous, so the rows of a sample are h * w of the merged
    map.  row_scale=None: every launch is the one it always was."""
    if row_scale is not None:
        if pool or defer_apply or act is not None:
            raise NotImplementedError('conv_bn_act(row_scale=...): no pool, defer_apply or act= (a ReLU residual unit only)')
        if bn is None or not relu or shortcut is None or x.data.dim() != 4:
            raise ValueError('conv_bn_act(row_scale=...): BatchNorm + ReLU + shortcut on a 4-D input')
        samples = x.shape[0] // (x.phase * x.phase)
        if row_scale.dtype != F32 or row_scale.dim() != 1 or row_scale.numel() != samples or not row_scale.is_contiguous():
            raise ValueError(f'conv_bn_act(row_scale=...): a contiguous fp32 vector of {samples} factors (one per sample), got '
                             f'{row_scale.dtype} {tuple(row_scale.shape)}')
    if pool and (bn is None or not relu or shortcut is not None or x.data.dim() != 4):
        raise ValueError('conv_bn_act(pool=True): BatchNorm + ReLU on a 4-D input, no shortcut')
    if (isinstance(conv, nn.Conv2d) and _is_grouped(conv) and bn is not None and shortcut is None and not pool
            and not defer_apply):
        return gconv_bn_act(region, x, conv, bn, relu=relu, act=act)       # (anything else grouped: _check_conv refuses below)
    act = _check_act(relu, act, bn, shortcut, pool, defer_apply)
    relu = act == RELU
    phase = x.phase
    if phase != 1:
        # a dilated stage in phase layout (phase_split): pointwise layers as they are, the dilated 3x3 as the padding-1 one
        # on the phase images; everything else is refused by await_ready (a dilation that is not the phase: by _check_conv)
        phased = _phased_conv_ok(conv, phase) and not pool and not defer_apply and x.data.dim() == 4
        if not phased and isinstance(conv, nn.Conv2d) and tuple(conv.dilation) != (1, 1):
            _check_conv(conv)
        await_ready(x, shortcut, phase_ok=phased)
        if shortcut is not None and shortcut.phase_steps != x.phase_steps:
            raise ValueError(f'conv_bn_act: the shortcut is in phase layout {shortcut.phase_steps or (1,)}, the unit in '
                             f'{x.phase_steps}: bring it there with phase_split / to_phase')
    else:
        await_ready(x, shortcut)
    lib, st = _C.lib(), stream_ptr()
    if isinstance(conv, nn.Linear):
        r = s = 1
        stride, pad = 1, 0
        k_real = conv.out_features
    else:
        _check_conv(conv, phase)
        r, s = conv.kernel_size
        stride, pad = conv.stride[0], conv.padding[0]
        k_real = conv.out_channels
        if phase != 1 and r == 3:
            pad = 1     # dilation == padding == phase on the merged map is padding 1 on every phase image
    if (SUBSAMPLE_S2 and r == 1 and s == 1 and stride == 2 and pad == 0 and x.data.dim() == 4 and not pool
            and x.rows() >= SUBSAMPLE_MIN_ROWS):
        # conv1x1/stride2(x) == conv1x1(x[:, ::2, ::2]): one strided copy, then a pointwise layer in all three passes
        x = subsample2(region, x)
        stride = 1
    x4 = x
    kp = pad8(k_real)
    if bn is not None and bn.num_features != k_real:
        raise ValueError(f'BatchNorm num_features {bn.num_features} != conv output channels {k_real}')
    if (FUSE_UNIT3 and bn is not None and act not in MASKLESS and (relu == (shortcut is not None)) and not pool
            and row_scale is None and isinstance(conv, nn.Conv2d)
            and r == 1 and s == 1 and stride == 1 and pad == 0 and conv.bias is None and x.data.dim() == 4
            and x.c == x.cp and kp == k_real and x.cp <= 1024 and (shortcut is None or shortcut.cp == kp)
            and x.rows() >= UNIT3_MIN_ROWS and kp >= 2 * x.cp
            and batch_stats(bn) and conv.weight.permute(0, 2, 3, 1).is_contiguous()):
        # the residual unit of a bottleneck (conv3 + bn3 + shortcut + ReLU) and its stride-1 projection shortcut (conv + bn):
        # normalise (add, activate) in the GEMM epilogue — the wide pre-BatchNorm tensor is never stored
        return _inherit_phase(_unit3_forward(region, x, conv, bn, shortcut, kp, relu), x)
    d = _conv_desc(x4, kp, r, s, stride, pad)
    training = region.grad_mode and (conv.weight.requires_grad or x.requires_grad or
                                     (bn is not None and bn.weight.requires_grad))
    pk = get_packs(conv.weight, conv.bias, kp, d.s_pad, x4.cp, want_dgrad=region.grad_mode and x.requires_grad,
                   refresh=True)
    dev = x.data.device
    y = torch.empty((d.n, d.p, d.q, kp), dtype=BF16, device=dev)
    m = d.n * d.p * d.q
    batch = bn is not None and batch_stats(bn)
    stats, rows = None, 0
    if batch:
        rows = lib.tok_conv_fwd_stat_rows(d)
        stats = torch.empty((2, rows, kp), dtype=F32, device=dev)
    node = _ConvBnActNode()
    _C.check(lib.tok_conv_fwd(d, ptr(x4.data), ptr(pk.fwd), ptr(pk.bias), ptr(y), ptr(stats), st), 'tok_conv_fwd')

    if bn is not None:
        scale, shift, mean, rstd = bn_coeffs(lib, st, bn, stats, rows, m, kp, dev)
        mask = cs_part = None
        deferred = bool(defer_apply and not relu and shortcut is None and not pool and x.data.dim() == 4)
        if deferred:
            out_data = y
        elif pool:
            p2, q2 = (d.p + 2 - 3) // 2 + 1, (d.q + 2 - 3) // 2 + 1
            out_data = torch.empty((d.n, p2, q2, kp), dtype=BF16, device=dev)
            node.pool = torch.empty((d.n, p2, q2, kp), dtype=torch.uint8, device=dev)
            if STEM_POOLED_STATS and region.grad_mode and batch:
                node.ypool = torch.empty_like(out_data)
            _C.check(lib.tok_bn_relu_maxpool_fwd(ptr(y), ptr(scale), ptr(shift), d.n, d.p, d.q, kp, ptr(out_data),
                                                 ptr(node.pool), ptr(node.ypool), st), 'tok_bn_relu_maxpool_fwd')
        elif (FUSE_UNIT3 and r == 3 and relu and shortcut is None and m >= UNIT3_MIN_ROWS
              and kp == k_real and kp <= 1024 and region.grad_mode and batch):
            # a 3x3 unit of a bottleneck feeds the fused residual unit, which wants colsum(z) of its input: the activation pass
            # has z in registers (saves that unit a stand-alone pass over z)
            out_data = torch.empty_like(y)
            mask = torch.empty((m, kp // 8), dtype=torch.uint8, device=dev)
            cs_rows = lib.tok_bn_act_fwd_colsum_rows(m, kp)
            cs_part = torch.empty((cs_rows, kp), dtype=F32, device=dev)
            _C.check(lib.tok_bn_act_fwd_colsum(ptr(y), ptr(scale), ptr(shift), None, 1, ptr(out_data), ptr(mask),
                                               m, kp, ptr(cs_part), st), 'tok_bn_act_fwd_colsum')
        else:
            # ReLU bits for the backward pass whenever gradients are on, running statistics included: the apply kernel's
            # mask-less fallback recomputes the pattern from y alone and would leave out a shortcut added before the activation
            out_data, mask = bn_apply(lib, st, y, scale, shift, act, shortcut, relu and region.grad_mode, m, kp, row_scale)
            node.row_scale = row_scale
        node.mask = mask
        node.mean, node.rstd, node.scale, node.shift = mean, rstd, scale, shift
    else:
        if relu or shortcut is not None:
            raise NotImplementedError('relu / shortcut without BatchNorm')
        out_data = y
    if x.data.dim() == 2:
        y = y.view(d.n, kp)
        out_data = out_data.view(d.n, kp)

    req = bool(training or (shortcut is not None and shortcut.requires_grad and region.grad_mode))
    out = _inherit_phase(TTensor(out_data, k_real, requires_grad=req), x)
    if bn is not None and deferred:
        out.affine = (scale, shift)
    if bn is not None and cs_part is not None:
        out.colsum_part = (cs_part, cs_rows)
    if req:
        node.x, node.out, node.shortcut, node.y = x, out, shortcut, y
        node.conv, node.bn, node.desc, node.pk = conv, bn, d, pk
        node.act, node.batch_stats = act, batch
        out.node = node
        node.sub_capable = False
        if x.requires_grad:
            x.uses += 1
            if (r == 1 and s == 1 and stride == 1 and pad == 0 and x.data.dim() == 4
                    and lib.tok_conv_dgrad_subacc_ok(d)):
                node.sub_capable = True      # this unit's data gradient can absorb a half-resolution contribution to d(x)
                x.sub_closers += 1
        if shortcut is not None and shortcut.requires_grad:
            shortcut.uses += 1
        region.add(node)
    return out


def linear(region: Region, x: TTensor, fc: nn.Linear) -> TTensor:
    """y = x W^T + b on the MFMA conv kernel (1x1, h = w = 1)."""
    return conv_bn_act(region, x, fc, None, False, None)


# ---- max pool ----------------------------------------------------------------------------------------

class _MaxPoolNode(Node):
    needs_backward = True

    def backward(self):
        g = self.out.grad
        if g is None or not self.x.requires_grad:
            return
        n, h, w, c = self.x.shape
        tgt, acc = grad_target(self.x)
        _C.check(_C.lib().tok_maxpool3x3s2_bwd(ptr(g), ptr(self.argmax), ptr(tgt), acc, n, h, w, c, stream_ptr()),
                 'tok_maxpool3x3s2_bwd')
        self.out.grad = None

    def release(self):
        self.x = self.out = self.argmax = None


def max_pool_3x3_s2(region: Region, x: TTensor) -> TTensor:
    refuse_phased(x, 'max_pool_3x3_s2')
    n, h, w, c = x.shape
    p, q = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    y = torch.empty((n, p, q, c), dtype=BF16, device=x.data.device)
    argmax = torch.empty((n, p, q, c), dtype=torch.uint8, device=x.data.device)
    _C.check(_C.lib().tok_maxpool3x3s2_fwd(ptr(x.data), ptr(y), ptr(argmax), n, h, w, c, stream_ptr()),
             'tok_maxpool3x3s2_fwd')
    req = region.grad_mode and x.requires_grad
    out = TTensor(y, x.c, requires_grad=req)
    if req:
        node = _MaxPoolNode()
        node.x, node.out, node.argmax = x, out, argmax
        out.node = node
        x.uses += 1
        region.add(node)
    return out


# ---- 2x2 average pool (avg_down shortcuts) ---------------------------------------------------------------------

class _Subsample2Node(Node):
    """x -> x[:, ::2, ::2]: the input of a 1x1 / stride-2 projection as a dense tensor.  Its backward does not touch d(x)
    when exactly one more contribution is due and that consumer's data gradient can absorb the half-resolution gradient
    in its epilogue (tok_conv_dgrad_subacc): the buffer is parked on `x.grad_sub`."""
    needs_backward = True

    def backward(self):
        g = self.out.grad
        x = self.x
        if g is None or not x.requires_grad:
            return
        self.out.grad = None
        if (x.grad is None and x.grad_sub is None and x.uses == 2 and x.arrived == 0 and x.sub_closers == 1
                and not getattr(_core_ms, 'active', False)):
            x.grad_sub = g
            x.arrived += 1
            return
        n, h, w, c = x.shape
        tgt, acc = grad_target(x)
        _C.check(_C.lib().tok_subsample2_bwd(ptr(g), n, h, w, c, ptr(tgt), acc, stream_ptr()), 'tok_subsample2_bwd')

    def release(self):
        self.x = self.out = None


# 1x1 / stride-2 / no-padding convolutions run as pointwise layers on the subsampled input (forward, weight gradient, data
# gradient on the streaming kernels; the unit-3 fusion applies to the projection + BatchNorm).  Measured on ResNet-50 B=256:
# see DESIGN.md section 8.
SUBSAMPLE_S2 = os.environ.get('TOK_SUBSAMPLE_S2', '1') != '0'
# rows of the full-resolution input (round 6: 100 000 -> 40 000 puts ResNet-50's layer4.0 projection at batch 256 — 50 176 rows, the
# last stride-2 1x1 data gradient on the parity-class kernel — on the subsampled plan too: 17.42 vs 17.50 ms/step, two same-box rounds)
SUBSAMPLE_MIN_ROWS = int(os.environ.get('TOK_SUBSAMPLE_MIN_ROWS', '40000'))


def subsample2(region: Region, x: TTensor) -> TTensor:
    refuse_phased(x, 'subsample2')
    n, h, w, c = x.shape
    y = torch.empty((n, (h + 1) // 2, (w + 1) // 2, c), dtype=BF16, device=x.data.device)
    _C.check(_C.lib().tok_subsample2_fwd(ptr(x.data), n, h, w, c, ptr(y), stream_ptr()), 'tok_subsample2_fwd')
    req = region.grad_mode and x.requires_grad
    out = TTensor(y, x.c, requires_grad=req)
    if req:
        node = _Subsample2Node()
        node.x, node.out = x, out
        out.node = node
        x.uses += 1
        region.add(node)
    return out


# ---- phase layout (space-to-batch): how a dilated stage runs on the plain kernels -----------------------------------------
# A 3x3 / stride-1 convolution with dilation d and padding d is the plain 3x3 / padding-1 convolution on each of the d x d
# phase images x[:, a::d, b::d, :] (zero padding by d in the image is zero padding by 1 in every phase image), and 1x1
# convolutions, BatchNorm, ReLU and the residual add do not care which pixel is where.  phase_split turns an (N, H, W, C)
# tensor into the N * d * d phase images (N * d * d, H / d, W / d, C), image (i, a, b) at index (i * d + a) * d + b, and a whole
# dilated stage runs on them; phase_merge is the inverse (csrc/phase.hip).
# Nested splits: a split sees the tensor it is given as a batch of images, so splitting a phase-2 tensor by 2 gives phase 4 with
# image index ((i * 2 + a1) * 2 + b1) * 4 + a2 * 2 + b2 for the pixels Y = 4y + 2 * a2 + a1, X = 4x + 2 * b2 + b1: the INNER
# split holds the higher bit.  Each of those images is a phase image of dilation 4, but their order is not that of one split
# by 4 — TTensor.phase_steps, (2, 2) against (4,), keeps the two apart, and a merge undoes the LAST split only.

class _PhaseNode(Node):
    """A split or a merge; its backward is the other kernel on the output gradient, into grad_target(x) (= or +=)."""
    needs_backward = True

    def backward(self):
        g = self.out.grad
        if g is None or not self.x.requires_grad:
            return
        self.out.grad = None
        tgt, acc = grad_target(self.x)
        n, h, w, c, d = self.geo
        fn, name = (_C.lib().tok_phase_merge, 'tok_phase_merge') if self.split else (_C.lib().tok_phase_split, 'tok_phase_split')
        _C.check(fn(ptr(g), n, h, w, c, c, d, ptr(tgt), acc, stream_ptr()), name)

    def release(self):
        self.x = self.out = None


def _phase_move(region: Region, x: TTensor, d: int, split: bool) -> TTensor:
    if d not in (2, 4):
        raise NotImplementedError(f'phase_{"split" if split else "merge"}: d = {d}, 2 or 4 are served')
    await_ready(x, phase_ok=True)
    if x.data.dim() != 4 or x.affine is not None:
        raise NotImplementedError('phase_split / phase_merge: a 4-D tensor without a deferred BatchNorm apply')
    nb, hb, wb, c = x.shape
    if split:
        n, h, w = nb, hb, wb                         # the sizes of the MERGED tensor of this call
        if h % d or w % d:
            raise NotImplementedError(f'phase_split: a map of h = {h}, w = {w} is not divisible by d = {d} (a dilated stage '
                                      f'needs an input whose map at that stage is a multiple of its dilation)')
        shape, steps = (n * d * d, h // d, w // d, c), x.phase_steps + (d,)
    else:
        if not x.phase_steps or x.phase_steps[-1] != d:
            raise ValueError(f'phase_merge by {d}: the last split of this tensor is {x.phase_steps[-1:] or None} '
                             f'(phase_steps {x.phase_steps})')
        n, h, w = nb // (d * d), hb * d, wb * d
        shape, steps = (n, h, w, c), x.phase_steps[:-1]
    y = torch.empty(shape, dtype=BF16, device=x.data.device)
    fn, name = (_C.lib().tok_phase_split, 'tok_phase_split') if split else (_C.lib().tok_phase_merge, 'tok_phase_merge')
    _C.check(fn(ptr(x.data), n, h, w, c, c, d, ptr(y), 0, stream_ptr()), name)
    req = region.grad_mode and x.requires_grad
    out = TTensor(y, x.c, requires_grad=req)
    out.phase_steps = steps
    for f in steps:
        out.phase *= f
    if req:
        node = _PhaseNode()
        node.x, node.out, node.split, node.geo = x, out, split, (n, h, w, c, d)
        out.node = node
        x.uses += 1
        region.add(node)
    return out


def phase_split(region: Region, x: TTensor, d: int) -> TTensor:
    """x -> its d x d phase images (see above); a phase-2 tensor split by 2 gives phase 4.  h or w not divisible by d:
    NotImplementedError before anything is launched."""
    return _phase_move(region, x, d, True)


def phase_merge(region: Region, x: TTensor, d: int) -> TTensor:
    """Undo the last split of x, which must have been by d: phase 4 = (2, 2) -> phase 2 -> phase 1."""
    return _phase_move(region, x, d, False)


def to_phase(region: Region, x: TTensor, d: int) -> TTensor:
    """x in phase d: x itself when it is there already, split upward otherwise (never merged implicitly)."""
    if x.phase == d:
        return x
    if d % x.phase or d // x.phase not in (2, 4):
        raise ValueError(f'to_phase: phase {x.phase} -> {d} is no split by 2 or 4 (merge explicitly with phase_merge)')
    return phase_split(region, x, d // x.phase)


def from_phase(region: Region, x: TTensor) -> TTensor:
    """x in plain layout: every split undone, last one first (x itself when it is plain)."""
    while x.phase != 1:
        x = phase_merge(region, x, x.phase_steps[-1])
    return x


class _AvgPool2Node(Node):
    needs_backward = True

    def backward(self):
        g = self.out.grad
        if g is None or not self.x.requires_grad:
            return
        n, h, w, c = self.x.shape
        tgt, acc = grad_target(self.x)
        _C.check(_C.lib().tok_avgpool2x2_bwd(ptr(g), ptr(tgt), acc, n, h, w, c, stream_ptr()), 'tok_avgpool2x2_bwd')
        self.out.grad = None

    def release(self):
        self.x = self.out = None


def avg_pool_2x2(region: Region, x: TTensor) -> TTensor:
    """AvgPool2d(2, stride 2, ceil_mode=True, count_include_pad=False) ([timm] downsample_avg)."""
    await_ready(x)       # x may come from a branch stream
    n, h, w, c = x.shape
    y = torch.empty((n, (h + 1) // 2, (w + 1) // 2, c), dtype=BF16, device=x.data.device)
    _C.check(_C.lib().tok_avgpool2x2_fwd(ptr(x.data), ptr(y), n, h, w, c, stream_ptr()), 'tok_avgpool2x2_fwd')
    req = region.grad_mode and x.requires_grad
    out = TTensor(y, x.c, requires_grad=req)
    if req:
        node = _AvgPool2Node()
        node.x, node.out = x, out
        out.node = node
        x.uses += 1
        region.add(node)
    return out


# ---- global average pool --------------------------------------------------------------------------------

class _GapNode(Node):
    needs_backward = True

    def backward(self):
        g = self.out.grad
        if g is None or not self.x.requires_grad:
            return
        n, h, w, c = self.x.shape
        tgt, acc = grad_target(self.x)
        _C.check(_C.lib().tok_gap_bwd(ptr(g), ptr(tgt), acc, n, h * w, c, stream_ptr()), 'tok_gap_bwd')
        self.out.grad = None

    def release(self):
        self.x = self.out = None


def global_avg_pool(region: Region, x: TTensor) -> TTensor:
    refuse_phased(x, 'global_avg_pool')
    n, h, w, c = x.shape
    y = torch.empty((n, c), dtype=BF16, device=x.data.device)
    _C.check(_C.lib().tok_gap_fwd(ptr(x.data), ptr(y), n, h * w, c, stream_ptr()), 'tok_gap_fwd')
    req = region.grad_mode and x.requires_grad
    out = TTensor(y, x.c, requires_grad=req)
    if req:
        node = _GapNode()
        node.x, node.out = x, out
        out.node = node
        x.uses += 1
        region.add(node)
    return out


# ---- global max / avgmax / catavgmax pool ------------------------------------------------------------------

POOL_MODES = {'max': 1, 'avgmax': 2, 'catavgmax': 3}


class _GlobalPoolNode(Node):
    needs_backward = True

    def backward(self):
        g = self.out.grad
        if g is None or not self.x.requires_grad:
            return
        n, h, w, c = self.x.shape
        tgt, acc = grad_target(self.x)
        _C.check(_C.lib().tok_global_pool_bwd(ptr(g), ptr(self.argmax), ptr(tgt), acc, n, h * w, c, g.shape[-1], self.mode,
                                              stream_ptr()), 'tok_global_pool_bwd')
        self.out.grad = None

    def release(self):
        self.x = self.out = self.argmax = None


def global_pool(region: Region, x: TTensor, pool_type: str) -> TTensor:
    """SelectAdaptivePool2d(1, pool_type, flatten=True) ([timm], reference pooling.py:7-12): 'avg', 'max',
    'avgmax' = 0.5 * (avg + max), 'catavgmax' = cat(avg, max) along channels."""
    if pool_type == 'avg':
        return global_avg_pool(region, x)
    mode = POOL_MODES[pool_type]
    refuse_phased(x, 'global_pool')
    n, h, w, c = x.shape
    if mode == 3 and x.c != c:
        raise NotImplementedError("torchok_amd Pooling 'catavgmax': channel counts that are multiples of 8")
    cout = 2 * c if mode == 3 else c
    y = torch.empty((n, cout), dtype=BF16, device=x.data.device)
    argmax = torch.empty((n, c), dtype=torch.int32, device=x.data.device)
    _C.check(_C.lib().tok_global_pool_fwd(ptr(x.data), ptr(y), ptr(argmax), n, h * w, c, cout, mode, stream_ptr()),
             'tok_global_pool_fwd')
    req = region.grad_mode and x.requires_grad
    out = TTensor(y, 2 * x.c if mode == 3 else x.c, requires_grad=req)
    if req:
        node = _GlobalPoolNode()
        node.x, node.out, node.argmax, node.mode = x, out, argmax, mode
        out.node = node
        x.uses += 1
        region.add(node)
    return out


# ---- depthwise conv + bn + relu (MnasNet) --------------------------------------------------------------------------------

def _check_dwconv(conv: nn.Conv2d, x: TTensor):
    k = conv.kernel_size[0]
    if (conv.groups != conv.in_channels or conv.out_channels != conv.in_channels or conv.bias is not None
            or conv.kernel_size != (k, k) or k not in (3, 5) or tuple(conv.stride) not in ((1, 1), (2, 2))
            or tuple(conv.padding) != (k // 2, k // 2) or tuple(conv.dilation) != (1, 1) or conv.padding_mode != 'zeros'):
        raise NotImplementedError('torchok_amd depthwise conv: groups == channels, no bias, k in {3, 5}, stride 1 or 2, '
                                  'padding k // 2, no dilation')
    if x.data.dim() != 4 or x.c != x.cp or x.c != conv.in_channels:
        raise NotImplementedError('torchok_amd depthwise conv: a 4-D input whose channel count is a multiple of 8')


class _SameWidthConvBnActNode(_ConvBnActNode):
    """act(bn(conv(x))) for a convolution with as many output as input channels that has kernels of its own (depthwise,
    grouped 3x3).  The BatchNorm backward is the one of _ConvBnActNode (tok_bn_bwd_*; a consumer conv's data gradient may
    reduce its sums, see wants_fused_bwd_stats); then the family's weight and data gradient on dy.  A family states its five
    library calls; `geo` is (n, h, w, c, c, kernel size | groups, stride), the sizes every one of them takes."""

    # -- what a family provides (the weight is read, and its gradient written, as the master lies in memory) --
    @staticmethod
    def stat_rows(lib, conv, geo): raise NotImplementedError

    @staticmethod
    def launch_fwd(lib, conv, geo, x, y, stats, st): raise NotImplementedError

    @staticmethod
    def wgrad_ws_bytes(lib, conv, geo): raise NotImplementedError

    @staticmethod
    def launch_wgrad(lib, conv, geo, x, dy, slot, acc, ws, ws_bytes, st): raise NotImplementedError

    @staticmethod
    def launch_dgrad(lib, conv, geo, dy, tgt, acc, st): raise NotImplementedError

    @staticmethod
    def geo(conv, x: TTensor):
        n, h, w, c = x.shape
        return n, h, w, c, c, conv.kernel_size[0], conv.stride[0]

    def backward(self):
        lib, st = _C.lib(), stream_ptr()
        out: TTensor = self.out
        g = out.grad
        if g is None:
            return
        conv, x = self.conv, self.x
        geo = self.geo(conv, x)
        m, kp = self.y.numel() // self.y.shape[-1], self.y.shape[-1]
        w_need, x_need = conv.weight.requires_grad, x.requires_grad
        dy = self._bn_bwd(lib, st, g, m, kp, w_need or x_need)
        out.grad = None
        if dy is None:
            return
        if w_need:
            ws_bytes = self.wgrad_ws_bytes(lib, conv, geo)
            ws = torch.empty(max(ws_bytes // 4, 1), dtype=F32, device=g.device)
            slot, acc = PG.sink(conv.weight)
            self.launch_wgrad(lib, conv, geo, x.data, dy, slot, acc, ws, ws_bytes, st)
            PG.commit(conv.weight, slot, acc)
        if x_need:
            tgt, acc = grad_target(x)
            self.launch_dgrad(lib, conv, geo, dy, tgt, acc, st)


def _same_width_conv_bn_act(node_cls, region: Region, x: TTensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, act,
                            phase_ok: bool = False) -> TTensor:
    """The forward of a _SameWidthConvBnActNode family (the caller has checked the layer and resolved `act`; a family that
    takes an input in phase layout has checked that too: the unit then runs on the phase images)."""
    await_ready(x, phase_ok=phase_ok)
    if bn.num_features != conv.out_channels:
        raise ValueError(f'BatchNorm num_features {bn.num_features} != conv output channels {conv.out_channels}')
    lib, st = _C.lib(), stream_ptr()
    geo = node_cls.geo(conv, x)
    n, h, w, c, stride = geo[0], geo[1], geo[2], geo[3], geo[-1]
    p, q = (h - 1) // stride + 1, (w - 1) // stride + 1
    dev = x.data.device
    batch = batch_stats(bn)
    y = torch.empty((n, p, q, c), dtype=BF16, device=dev)
    stats, rows = None, 0
    if batch:
        rows = node_cls.stat_rows(lib, conv, geo)
        stats = torch.empty((2, rows, c), dtype=F32, device=dev)
    node_cls.launch_fwd(lib, conv, geo, x.data, y, stats, st)
    m = n * p * q
    scale, shift, mean, rstd = bn_coeffs(lib, st, bn, stats, rows, m, c, dev)
    training = region.grad_mode and (conv.weight.requires_grad or x.requires_grad or bn.weight.requires_grad
                                     or bn.bias.requires_grad)
    out_data, mask = bn_apply(lib, st, y, scale, shift, act, None, act == RELU and training, m, c)
    out = _inherit_phase(TTensor(out_data, c, requires_grad=bool(training)), x)
    if training:
        node = node_cls()
        node.x, node.out, node.y, node.mask = x, out, y, mask
        node.conv, node.bn, node.act, node.batch_stats = conv, bn, act, batch
        node.mean, node.rstd, node.scale, node.shift = mean, rstd, scale, shift
        out.node = node
        if x.requires_grad:
            x.uses += 1
        region.add(node)
    return out


class _DwConvBnActNode(_SameWidthConvBnActNode):
    """relu(bn(depthwise_conv(x))) on tok_dwconv_*; geo[5] is the kernel size."""

    @staticmethod
    def stat_rows(lib, conv, geo):
        n, h, w, c, _, k, stride = geo
        return lib.tok_dwconv_rows(n, h, w, c, k, stride)

    @staticmethod
    def launch_fwd(lib, conv, geo, x, y, stats, st):
        _C.check(lib.tok_dwconv_fwd(ptr(x), ptr(conv.weight), *geo, ptr(y), ptr(stats), st), 'tok_dwconv_fwd')

    @staticmethod
    def wgrad_ws_bytes(lib, conv, geo):
        n, h, w, c, _, k, stride = geo
        return lib.tok_dwconv_wgrad_ws_bytes(n, h, w, c, k, stride)

    @staticmethod
    def launch_wgrad(lib, conv, geo, x, dy, slot, acc, ws, ws_bytes, st):
        _C.check(lib.tok_dwconv_wgrad(ptr(x), ptr(dy), *geo, ptr(slot), acc, ptr(ws), ws_bytes, st), 'tok_dwconv_wgrad')

    @staticmethod
    def launch_dgrad(lib, conv, geo, dy, tgt, acc, st):
        _C.check(lib.tok_dwconv_dgrad(ptr(dy), ptr(conv.weight), *geo, ptr(tgt), acc, st), 'tok_dwconv_dgrad')


def dwconv_bn_act(region: Region, x: TTensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, relu: bool = True,
                  act: Optional[str] = None) -> TTensor:
    """out = act(bn(conv(x))) for a depthwise `conv` ([timm] create_conv2d(depthwise=True) + BatchNormAct2d of the MnasNet
    and MobileNetV3 blocks).  act=None: `relu` decides; act='hard_swish' / 'relu6': as in conv_bn_act.  Training-mode BatchNorm takes its statistics from the convolution launch (tok_dwconv_fwd leaves the partial
    rows tok_bn_finalize folds); eval mode uses the running statistics; track_running_stats=False uses batch statistics."""
    act = _check_act(relu, act, bn)
    _check_dwconv(conv, x)
    return _same_width_conv_bn_act(_DwConvBnActNode, region, x, conv, bn, act)


# ---- grouped 3x3 conv + bn + relu (ResNeXt) ------------------------------------------------------------------------------

GCONV_WIDTHS = (4, 8, 16, 32, 64)      # group widths csrc/conv_group.hip serves


def _is_grouped(conv: nn.Conv2d) -> bool:
    """A grouped convolution that is neither dense nor depthwise: the grouped unit's to serve or to refuse."""
    return conv.groups > 1 and conv.groups != conv.in_channels


def _check_gconv(conv: nn.Conv2d, x: TTensor):
    g = conv.groups
    if (g < 2 or conv.in_channels != conv.out_channels or conv.in_channels % g != 0 or conv.in_channels // g not in GCONV_WIDTHS
            or conv.bias is not None or conv.kernel_size != (3, 3) or tuple(conv.stride) not in ((1, 1), (2, 2))
            or conv.padding_mode != 'zeros'
            or (tuple(conv.padding) != (1, 1) or tuple(conv.dilation) != (1, 1) if x.phase == 1 else not _phased_conv_ok(conv, x.phase))):
        raise NotImplementedError(f'torchok_amd grouped conv: 3x3, groups >= 2, as many output as input channels, group width '
                                  f'in {GCONV_WIDTHS}, no bias, stride 1 or 2, padding 1, no dilation')
    if x.data.dim() != 4 or x.c != x.cp or x.c != conv.in_channels:
        raise NotImplementedError('torchok_amd grouped conv: a 4-D input whose channel count is a multiple of 8')


def _w_krsc(weight: torch.Tensor) -> int:
    """Which of the two layouts tok_gconv_* reads the (K, cg, 3, 3) master (and writes its gradient slot) in: 1 channels-last
    [k][3][3][cg], 0 [k][cg][3][3]."""
    if weight.is_contiguous():
        return 0
    if weight.permute(0, 2, 3, 1).is_contiguous():
        return 1
    raise RuntimeError('grouped conv weight must be contiguous or channels-last')


class _GConvBnActNode(_SameWidthConvBnActNode):
    """relu(bn(grouped_conv(x))) on tok_gconv_*; geo[5] is the number of groups.  The gradient slot has the master's strides, so
    one layout flag serves the weight and its gradient."""

    @staticmethod
    def geo(conv, x: TTensor):
        n, h, w, c = x.shape
        return n, h, w, c, c, conv.groups, conv.stride[0]

    @staticmethod
    def stat_rows(lib, conv, geo):
        n, h, w, c, _, groups, stride = geo
        return lib.tok_gconv_rows(n, h, w, c, groups, stride)

    @staticmethod
    def launch_fwd(lib, conv, geo, x, y, stats, st):
        _C.check(lib.tok_gconv_fwd(ptr(x), ptr(conv.weight), _w_krsc(conv.weight), *geo, ptr(y), ptr(stats), st), 'tok_gconv_fwd')

    @staticmethod
    def wgrad_ws_bytes(lib, conv, geo):
        n, h, w, c, _, groups, stride = geo
        return lib.tok_gconv_wgrad_ws_bytes(n, h, w, c, groups, stride)

    @staticmethod
    def launch_wgrad(lib, conv, geo, x, dy, slot, acc, ws, ws_bytes, st):
        _C.check(lib.tok_gconv_wgrad(ptr(x), ptr(dy), *geo, ptr(slot), _w_krsc(conv.weight), acc, ptr(ws), ws_bytes, st),
                 'tok_gconv_wgrad')

    @staticmethod
    def launch_dgrad(lib, conv, geo, dy, tgt, acc, st):
        _C.check(lib.tok_gconv_dgrad(ptr(dy), ptr(conv.weight), _w_krsc(conv.weight), *geo, ptr(tgt), acc, st), 'tok_gconv_dgrad')


def gconv_bn_act(region: Region, x: TTensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, relu: bool = True,
                 act: Optional[str] = None) -> TTensor:
    """out = act(bn(conv(x))) for a grouped 3x3 `conv` ([timm] Bottleneck.conv2 + bn2 + act2 of the ResNeXts).  act=None: `relu`
    decides; act='hard_swish' / 'relu6': as in conv_bn_act.  The kernels read the fp32 master itself (rounded to bf16 as a wave builds its
    fragments): there is no packed copy that an optimizer step could leave stale.  The BatchNorm stage is dwconv_bn_act's.  An
    input in phase layout (phase_split) is served when the layer's stride is 1 and its dilation and padding equal the phase: the
    kernels then run on the phase images as the padding-1 convolution they always are.  The
    output carries no `colsum_part`: a fused residual unit that consumes it sums the columns itself (_unit3_forward)."""
    act = _check_act(relu, act, bn)
    _check_gconv(conv, x)
    return _same_width_conv_bn_act(_GConvBnActNode, region, x, conv, bn, act, phase_ok=True)


# ---- squeeze-excite (MnasNet-A1) -----------------------------------------------------------------------------------------

SE_GATES = {'sigmoid': 0, 'hard_sigmoid': 1}      # gate_kind of tok_se_gate_fwd / _bwd
SE_ACTS = {'relu': 0, 'gelu': 1}                  # act_kind of tok_se_act_fwd / _bwd


class _SqueezeExciteNode(Node):
    needs_backward = True
    gate_kind = 0
    act_kind = 0            # SE_ACTS: the activation between the two 1x1 layers

    def backward(self):
        g = self.out.grad
        if g is None:
            return
        self.out.grad = None
        se, x = self.se, self.x
        lib = _C.lib()
        n, h, w, c = x.shape
        red, exp = self.layers
        rd = red.out_channels
        prm = (red.weight, red.bias, exp.weight, exp.bias)
        targets = [(p, *(PG.sink(p) if p is not None and p.requires_grad else (None, 0))) for p in prm]
        acc_bits = sum(acc << bit for bit, (_, _, acc) in enumerate(targets))
        dx, dx_acc = grad_target(x) if x.requires_grad else (None, 0)
        general = self.act_kind != 0 or red.bias is None
        ws = torch.empty((lib.tok_se_act_ws_floats if general else lib.tok_se_ws_floats)(n, h * w, c, rd), dtype=F32,
                         device=g.device)
        if general:
            _C.check(lib.tok_se_act_bwd(ptr(g), ptr(x.data), n, h * w, c, c, rd, self.gate_kind, self.act_kind, ptr(prm[0]),
                                        ptr(prm[2]), ptr(self.mean), ptr(self.hid), ptr(self.gate),
                                        *(ptr(t[1]) for t in targets), acc_bits, ptr(dx), dx_acc, ptr(ws), stream_ptr()),
                     'tok_se_act_bwd')
        elif self.gate_kind:
            _C.check(lib.tok_se_gate_bwd(ptr(g), ptr(x.data), n, h * w, c, c, rd, self.gate_kind, ptr(prm[0]), ptr(prm[2]),
                                         ptr(self.mean), ptr(self.hid), ptr(self.gate), *(ptr(t[1]) for t in targets), acc_bits,
                                         ptr(dx), dx_acc, ptr(ws), stream_ptr()), 'tok_se_gate_bwd')
        else:
            _C.check(lib.tok_se_bwd(ptr(g), ptr(x.data), n, h * w, c, c, rd, ptr(prm[0]), ptr(prm[2]), ptr(self.mean),
                                    ptr(self.hid), ptr(self.gate), *(ptr(t[1]) for t in targets), acc_bits, ptr(dx), dx_acc,
                                    ptr(ws), stream_ptr()), 'tok_se_bwd')
        for p, slot, acc in targets:
            if slot is not None:
                PG.commit(p, slot, acc)
        if self.region is not None:
            self.region.keep_until_join(ws)

    def release(self):
        self.x = self.out = self.mean = self.hid = self.gate = self.layers = None


def squeeze_excite(region: Region, x: TTensor, se: nn.Module, gate: str = 'sigmoid', act: str = 'relu',
                   names: Tuple[str, str] = ('conv_reduce', 'conv_expand')) -> TTensor:
    """x * gate(conv_expand(act(conv_reduce(mean_hw(x)))))  ([timm] efficientnet_blocks.SqueezeExcite with ReLU inside and
    the 'sigmoid' (MnasNet) or 'hard_sigmoid' (MobileNetV3) gate).  `se` holds conv_reduce / conv_expand (1x1, with bias) as
    parameter containers.  act='gelu' and / or two layers without bias ([timm 0.6.13] SEModule as GCViT's MbConvBlock builds it,
    names=('fc1', 'fc2')) go through tok_se_act_fwd / _bwd; the defaults are the launches they have always been."""
    if gate not in SE_GATES:
        raise NotImplementedError(f'torchok_amd squeeze-excite gate {gate!r}: one of {sorted(SE_GATES)}')
    if act not in SE_ACTS:
        raise NotImplementedError(f'torchok_amd squeeze-excite activation {act!r}: one of {sorted(SE_ACTS)}')
    gate_kind, act_kind = SE_GATES[gate], SE_ACTS[act]
    await_ready(x)
    red, exp = getattr(se, names[0]), getattr(se, names[1])
    general = act_kind != 0 or (red.bias is None and exp.bias is None)
    if x.data.dim() != 4 or x.c != x.cp or red.in_channels != x.c or exp.out_channels != x.c \
            or red.out_channels != exp.in_channels or (red.bias is None) != (exp.bias is None) \
            or (red.bias is None and not general):
        raise NotImplementedError('torchok_amd squeeze-excite: 1x1 convs with bias around a 4-D input of 8k channels')
    lib, st = _C.lib(), stream_ptr()
    n, h, w, c = x.shape
    rd = red.out_channels
    dev = x.data.device
    w1, w2 = red.weight, exp.weight
    if not (w1.is_contiguous() or w1.permute(0, 2, 3, 1).is_contiguous()) or \
            not (w2.is_contiguous() or w2.permute(0, 2, 3, 1).is_contiguous()):
        raise NotImplementedError('torchok_amd squeeze-excite: dense 1x1 weights')
    mean = torch.empty((n, c), dtype=F32, device=dev)
    hid = torch.empty((n, rd), dtype=F32, device=dev)
    gate_v = torch.empty((n, c), dtype=F32, device=dev)
    ws = torch.empty((lib.tok_se_act_ws_floats if general else lib.tok_se_ws_floats)(n, h * w, c, rd), dtype=F32, device=dev)
    if general:
        _C.check(lib.tok_se_act_fwd(ptr(x.data), n, h * w, c, c, rd, gate_kind, act_kind, ptr(w1), ptr(red.bias), ptr(w2),
                                    ptr(exp.bias), ptr(mean), ptr(hid), ptr(gate_v), ptr(ws), st), 'tok_se_act_fwd')
    elif gate_kind:
        _C.check(lib.tok_se_gate_fwd(ptr(x.data), n, h * w, c, c, rd, gate_kind, ptr(w1), ptr(red.bias), ptr(w2), ptr(exp.bias),
                                     ptr(mean), ptr(hid), ptr(gate_v), ptr(ws), st), 'tok_se_gate_fwd')
    else:
        _C.check(lib.tok_se_fwd(ptr(x.data), n, h * w, c, c, rd, ptr(w1), ptr(red.bias), ptr(w2), ptr(exp.bias), ptr(mean),
                                ptr(hid), ptr(gate_v), ptr(ws), st), 'tok_se_fwd')
    out_data = torch.empty_like(x.data)
    _C.check(lib.tok_channel_scale(ptr(x.data), ptr(gate_v), ptr(out_data), 0, n, h * w, c, c, st), 'tok_channel_scale')
    req = region.grad_mode and (x.requires_grad or any(p.requires_grad for p in se.parameters()))
    out = TTensor(out_data, c, requires_grad=bool(req))
    if req:
        node = _SqueezeExciteNode()
        node.x, node.out, node.se, node.mean, node.hid, node.gate = x, out, se, mean, hid, gate_v
        node.layers = (red, exp)
        if gate_kind:
            node.gate_kind = gate_kind
        if act_kind:
            node.act_kind = act_kind
        out.node = node
        if x.requires_grad:
            x.uses += 1
        region.add(node)
    return out


# ---- efficient channel attention + residual (ECA-ResNet) ----------------------------------------------------------------

class _EcaResidualNode(Node):
    needs_backward = True

    def backward(self):
        g = self.out.grad
        if g is None:
            return
        self.out.grad = None
        z, sc, w = self.z, self.shortcut, self.se.conv.weight
        lib = _C.lib()
        n, h, wd, c = z.shape
        dw, dw_acc = PG.sink(w) if w.requires_grad else (None, 0)
        dz, dz_acc = grad_target(z) if z.requires_grad else (None, 0)
        ds, ds_acc = grad_target(sc) if sc.requires_grad else (None, 0)
        ws = torch.empty(lib.tok_eca_ws_floats(n, h * wd, c), dtype=F32, device=g.device)
        _C.check(lib.tok_eca_bwd(ptr(g), ptr(self.out.data), ptr(z.data), n, h * wd, c, c, ptr(w), w.shape[-1], ptr(self.mean),
                                 ptr(self.gate), ptr(dw), dw_acc, ptr(dz), dz_acc, ptr(ds), ds_acc, ptr(ws), stream_ptr()),
                 'tok_eca_bwd')
        if dw is not None:
            PG.commit(w, dw, dw_acc)
        if self.region is not None:
            self.region.keep_until_join(ws)

    def release(self):
        self.z = self.shortcut = self.out = self.se = self.mean = self.gate = None


def eca_residual(region: Region, z: TTensor, se: nn.Module, shortcut: TTensor) -> TTensor:
    """relu(z * sigmoid(conv1d_k(mean_hw(z))) + shortcut)  ([timm 0.6.13] EcaModule as the `se` of a ResNet block, then the
    block's residual add and last activation).  `se.conv` is the nn.Conv1d(1, 1, k, padding=k // 2, bias=False) over the channel
    axis, a parameter container; z is the block's last BatchNorm output (conv_bn_act(..., relu=False))."""
    await_ready(z, shortcut)
    conv = se.conv
    k = conv.kernel_size[0] if isinstance(conv, nn.Conv1d) else 0
    if k == 0 or conv.in_channels != 1 or conv.out_channels != 1 or conv.bias is not None \
            or k % 2 != 1 or conv.padding[0] != k // 2 or conv.stride[0] != 1 or conv.dilation[0] != 1:
        raise NotImplementedError('torchok_amd ECA: nn.Conv1d(1, 1, k, padding=k // 2, bias=False) with odd k')
    if z.data.dim() != 4 or z.c != z.cp or shortcut.data.shape != z.data.shape or shortcut.c != z.c:
        raise NotImplementedError('torchok_amd ECA: a 4-D input of 8k channels and a shortcut of the same shape')
    lib, st = _C.lib(), stream_ptr()
    n, h, wd, c = z.shape
    dev = z.data.device
    w = conv.weight
    mean = torch.empty((n, c), dtype=F32, device=dev)
    gate = torch.empty((n, c), dtype=F32, device=dev)
    out_data = torch.empty_like(z.data)
    ws = torch.empty(lib.tok_eca_ws_floats(n, h * wd, c), dtype=F32, device=dev)
    _C.check(lib.tok_eca_fwd(ptr(z.data), ptr(shortcut.data), n, h * wd, c, c, ptr(w), k, ptr(mean), ptr(gate), ptr(out_data),
                             ptr(ws), st), 'tok_eca_fwd')
    req = bool(region.grad_mode and (z.requires_grad or shortcut.requires_grad or w.requires_grad))
    out = TTensor(out_data, c, requires_grad=req)
    if req:
        node = _EcaResidualNode()
        node.z, node.shortcut, node.out, node.se, node.mean, node.gate = z, shortcut, out, se, mean, gate
        out.node = node
        if z.requires_grad:
            z.uses += 1
        if shortcut.requires_grad:
            shortcut.uses += 1
        region.add(node)
    return out
