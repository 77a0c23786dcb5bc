"""The BatchNorm stage of every "producer -> BatchNorm -> activation" unit (conv_bn_act, dwconv_bn_act, gconv_bn_act, the commuted
neck).  A unit's FORM, chosen once by `choose_form` in its forward and kept on its node, states what differs between them."""
import torch

from .. import _C
from . import paramgrad as PG
from .core import donate_grad, grad_target, ptr

F32 = torch.float32
RELU, HARD_SWISH, RELU6 = 'relu', 'hard_swish', 'relu6'


def batch_stats(bn) -> bool:
    """Does this BatchNorm normalise with the statistics of the batch (training mode, or no running statistics kept)?"""
    return bn.training or bn.running_mean is None


def running_stat_ptrs(bn):
    """(running_mean, running_var, num_batches_tracked) for a finalize launch that updates them, three None when the module does
    not track them.  Cumulative-average BatchNorm is refused."""
    if bn.momentum is None:
        raise NotImplementedError('BatchNorm momentum=None (cumulative average)')
    if bn.training and bn.track_running_stats and bn.running_mean is not None:
        return ptr(bn.running_mean), ptr(bn.running_var), ptr(bn.num_batches_tracked)
    return None, None, None


def bn_coeffs(lib, st, bn, stats, rows, m, kp, dev):
    """(scale, shift, mean, rstd) per channel: from the producer's partial sums `stats` [2][rows][kp] over m rows (running
    statistics updated when the module tracks them), or, stats=None, from the running statistics (mean = rstd = None)."""
    # one allocation for the per-channel vectors (an allocator call costs the launch thread 2-3 us; HRNet-W48 makes 307
    # of these units per step)
    vec = torch.empty((4, kp), dtype=F32, device=dev)
    scale, shift, mean, rstd = vec.unbind()
    if stats is None:
        _C.check(lib.tok_bn_eval_coeffs(ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var),
                                        float(bn.eps), kp, bn.num_features, ptr(scale), ptr(shift), st), 'tok_bn_eval_coeffs')
        return scale, shift, None, None
    _C.check(lib.tok_bn_finalize(ptr(stats), rows, m, kp, bn.num_features, ptr(bn.weight), ptr(bn.bias), *running_stat_ptrs(bn),
                                 float(bn.momentum), float(bn.eps), ptr(mean), ptr(rstd), ptr(scale), ptr(shift), st),
             'tok_bn_finalize')
    return scale, shift, mean, rstd


# ---- the forms ----------------------------------------------------------------------------------------------------------
# fwd -> (out_data, mask, colsum_part); `want_mask` is the unit's rule for keeping the ReLU bits.  reduce / apply take the node `n`
# (y, mask, scale, shift, mean, rstd, out: what every unit has) and the gradient g of n.out: partial[2][rows][kp] = sum(dz),
# sum(dz * xhat); dy = c1*dz + c2*y + c3 (and the shortcut's dz).  Plain and Maskless hold no tensor and are shared; DropPath and
# StemPool are made per unit and own the tensors only they know (row_scale; argmax, ypool), released with the node's form.

class Plain:
    """out = act(y * scale + shift (+ shortcut)), act = identity or ReLU with its bit mask: tok_bn_act_fwd / tok_bn_bwd_*.
    colsums (ReLU, no shortcut): the activation pass, which has the values in registers, also leaves colsum(out) for a fused
    residual unit that reads out.  deferred (no activation): no apply pass, the consumer applies .affine = (scale, shift) itself.
    The apply launch can signal a completion event (tok_next_launch_event) and writes d(shortcut)."""
    carries_event = writes_shortcut = rider_ok = True   # (rider_ok: a data gradient's epilogue may reduce the sums)
    relu, colsums, deferred = 1, False, False       # (every form has them)

    def __init__(self, relu, colsums=False, deferred=False):
        self.relu, self.colsums, self.deferred = int(relu), colsums, deferred

    def fwd(self, lib, st, y, scale, shift, shortcut, want_mask, m, kp):
        if self.deferred:
            return y, None, None
        out = torch.empty_like(y)
        mask = torch.empty((m, kp // 8), dtype=torch.uint8, device=y.device) if want_mask or self.colsums else None
        sc = ptr(shortcut.data) if shortcut is not None else None
        if not self.colsums:
            _C.check(lib.tok_bn_act_fwd(ptr(y), ptr(scale), ptr(shift), sc, self.relu, ptr(out), ptr(mask), m, kp, st), 'tok_bn_act_fwd')
            return out, mask, None
        cs_rows = lib.tok_bn_act_fwd_colsum_rows(m, kp)
        cs_part = torch.empty((cs_rows, kp), dtype=F32, device=y.device)
        _C.check(lib.tok_bn_act_fwd_colsum(ptr(y), ptr(scale), ptr(shift), sc, self.relu, ptr(out), ptr(mask), m, kp, ptr(cs_part),
                                           st), 'tok_bn_act_fwd_colsum')
        return out, mask, (cs_part, cs_rows)

    def rows(self, lib, n, m, kp):
        return lib.tok_bn_bwd_rows(m, kp)

    def reduce(self, lib, st, n, g, m, kp, partial):
        _C.check(lib.tok_bn_bwd_reduce(ptr(g), ptr(n.y), ptr(n.mask), ptr(n.scale), ptr(n.shift), ptr(n.mean), ptr(n.rstd),
                                       self.relu, m, kp, ptr(partial), st), 'tok_bn_bwd_reduce')

    def apply(self, lib, st, n, g, coef, dy, ds_ptr, ds_acc, m, kp):
        _C.check(lib.tok_bn_bwd_apply(ptr(g), ptr(n.y), ptr(n.mask), ptr(n.scale), ptr(n.shift), ptr(coef), self.relu, ptr(dy),
                                      ds_ptr, ds_acc, m, kp, st), 'tok_bn_bwd_apply')


class Maskless(Plain):
    """Hard-swish or ReLU6 on tok_bn_<family>_fwd / _bwd_reduce / _bwd_apply: no mask (dz is recomputed from y), no shortcut."""
    carries_event = writes_shortcut = rider_ok = False

    def __init__(self, family):
        self.names = [f'tok_bn_{family}_{stage}' for stage in ('fwd', 'bwd_reduce', 'bwd_apply')]

    def fwd(self, lib, st, y, scale, shift, shortcut, want_mask, m, kp):
        out = torch.empty_like(y)
        _C.check(getattr(lib, self.names[0])(ptr(y), ptr(scale), ptr(shift), ptr(out), m, kp, st), self.names[0])
        return out, None, None

    def reduce(self, lib, st, n, g, m, kp, partial):
        _C.check(getattr(lib, self.names[1])(ptr(g), ptr(n.y), ptr(n.scale), ptr(n.shift), ptr(n.mean), ptr(n.rstd), m, kp,
                                             ptr(partial), st), self.names[1])

    def apply(self, lib, st, n, g, coef, dy, ds_ptr, ds_acc, m, kp):
        _C.check(getattr(lib, self.names[2])(ptr(g), ptr(n.y), ptr(n.scale), ptr(n.shift), ptr(coef), ptr(dy), m, kp, st),
                 self.names[2])


class DropPath(Plain):
    """Stochastic depth, a ReLU unit with a shortcut: out = relu(s[sample] * (y * scale + shift) + shortcut) on the
    tok_bn_droppath_* trio, the sample of a row being row // (m // len(s)).  Its dz is not mask * d(out): no rider."""
    rider_ok = False

    def __init__(self, row_scale):
        self.s, self.rps = row_scale, 0         # (rps: rows per sample, known in fwd)

    def fwd(self, lib, st, y, scale, shift, shortcut, want_mask, m, kp):
        out, self.rps = torch.empty_like(y), m // self.s.numel()
        mask = torch.empty((m, kp // 8), dtype=torch.uint8, device=y.device) if want_mask else None
        _C.check(lib.tok_bn_droppath_fwd(ptr(y), ptr(scale), ptr(shift), ptr(shortcut.data), ptr(self.s), self.rps,
                                         ptr(out), ptr(mask), m, kp, st), 'tok_bn_droppath_fwd')
        return out, mask, None

    def reduce(self, lib, st, n, g, m, kp, partial):
        _C.check(lib.tok_bn_droppath_bwd_reduce(ptr(g), ptr(n.y), ptr(n.mask), ptr(self.s), self.rps, ptr(n.mean),
                                                ptr(n.rstd), m, kp, ptr(partial), st), 'tok_bn_droppath_bwd_reduce')

    def apply(self, lib, st, n, g, coef, dy, ds_ptr, ds_acc, m, kp):
        _C.check(lib.tok_bn_droppath_bwd_apply(ptr(g), ptr(n.y), ptr(n.mask), ptr(self.s), self.rps, ptr(coef), ptr(dy),
                                               ds_ptr, ds_acc, m, kp, st), 'tok_bn_droppath_bwd_apply')


class StemPool(Plain):
    """out = maxpool3x3/s2/p1(relu(y * scale + shift)): `out` is the POOLED map and the activated one is never stored.  `argmax`
    holds the tap indices; `ypool` (keep_ypool) the raw conv output at the winning taps, for backward sums in the pooled domain."""
    carries_event = writes_shortcut = rider_ok = False

    def __init__(self, keep_ypool):
        self.keep_ypool, self.argmax, self.ypool = keep_ypool, None, None

    def fwd(self, lib, st, y, scale, shift, shortcut, want_mask, m, kp):
        n_, p, q, _ = y.shape
        out = torch.empty((n_, (p + 2 - 3) // 2 + 1, (q + 2 - 3) // 2 + 1, kp), dtype=y.dtype, device=y.device)
        self.argmax = torch.empty(out.shape, dtype=torch.uint8, device=y.device)
        self.ypool = torch.empty_like(out) if self.keep_ypool else None
        _C.check(lib.tok_bn_relu_maxpool_fwd(ptr(y), ptr(scale), ptr(shift), n_, p, q, kp, ptr(out), ptr(self.argmax),
                                             ptr(self.ypool), st), 'tok_bn_relu_maxpool_fwd')
        return out, None, None

    def rows(self, lib, n, m, kp):
        rows = lib.tok_bn_bwd_rows(m, kp)       # (asked in the position domain first, as it always was)
        return rows if self.ypool is None else lib.tok_bn_bwd_rows(n.out.data.numel() // kp, kp)

    def reduce(self, lib, st, n, g, m, kp, partial):
        if self.ypool is None:
            _C.check(lib.tok_bn_pool_bwd_reduce(ptr(g), ptr(self.argmax), ptr(n.y), ptr(n.scale), ptr(n.shift), ptr(n.mean),
                                                ptr(n.rstd), *n.y.shape[:3], kp, ptr(partial), st), 'tok_bn_pool_bwd_reduce')
            return
        # sums over the pooled elements (each feeds exactly one position): 3 pooled-size reads, no gather
        _C.check(lib.tok_bn_pool_bwd_reduce_pooled(ptr(g), ptr(n.out.data), ptr(self.ypool), ptr(n.mean), ptr(n.rstd),
                                                   n.out.data.numel() // kp, kp, ptr(partial), st), 'tok_bn_pool_bwd_reduce_pooled')

    def apply(self, lib, st, n, g, coef, dy, ds_ptr, ds_acc, m, kp):
        _C.check(lib.tok_bn_pool_bwd_apply(ptr(g), ptr(self.argmax), ptr(n.y), ptr(n.scale), ptr(n.shift), ptr(coef),
                                           *n.y.shape[:3], kp, ptr(dy), st), 'tok_bn_pool_bwd_apply')


MASKLESS = {HARD_SWISH: Maskless('hswish'), RELU6: Maskless('relu6')}     # the mask-less activations -> their form
_BY_ACT = {None: Plain(False), RELU: Plain(True), **MASKLESS}
_DEFERRED, _COLSUMS = Plain(False, deferred=True), Plain(True, colsums=True)


def choose_form(act, row_scale=None, pool=False, keep_ypool=False, deferred=False, colsums=False):
    """The form of a unit whose one activation is `act` (None / RELU / HARD_SWISH / RELU6): THE place where it is decided."""
    if pool:
        return StemPool(keep_ypool)
    if deferred or colsums:
        return _DEFERRED if deferred else _COLSUMS
    return DropPath(row_scale) if row_scale is not None else _BY_ACT[act]


def bn_apply(lib, st, y, scale, shift, act, shortcut, want_mask, m, kp, row_scale=None):
    """The apply pass out = act(y * scale + shift (+ shortcut)) -> (out_data, mask) of the form that `act` and `row_scale` choose."""
    return choose_form(act, row_scale).fwd(lib, st, y, scale, shift, shortcut, want_mask, m, kp)[:2]


def bn_backward(n, lib, st, g, m, kp, need_dy, side=False):
    """The BatchNorm (+ activation) backward of node `n` on the gradient g of n.out: dgamma / dbeta, then d(n.shortcut) and dy, the
    gradient of n.y (None when nobody needs it).  side: a weight gradient will be forked to the side stream behind the apply pass;
    where the form can, the pass carries the completion event itself (no event-record packet on the main queue) -> (dy, event)."""
    bn, form, sc = n.bn, n.form, n.shortcut
    g_need, b_need = bn.weight.requires_grad, bn.bias.requires_grad
    if n.batch_stats:
        if n.fused_partial is not None:
            partial, rows = n.fused_partial   # reduced by the dgrad that completed d(out)
        else:
            rows = form.rows(lib, n, m, kp)
            partial = torch.empty((2, rows, kp), dtype=F32, device=g.device)
            form.reduce(lib, st, n, g, m, kp, partial)
        coef = torch.empty((3, kp), dtype=F32, device=g.device)
        gbuf, bbuf, acc, finish = PG.pair_sinks(bn.weight if g_need else None, bn.bias if b_need else None)
        _C.check(lib.tok_bn_bwd_finalize(ptr(partial), rows, m, kp, bn.num_features, ptr(bn.weight), ptr(n.mean), ptr(n.rstd),
                                         ptr(gbuf), ptr(bbuf), ptr(coef), acc, int(n.fused_partial is not None), st),
                 'tok_bn_bwd_finalize')
        finish()
    else:
        # eval-mode BN: y -> out is a fixed affine map: dy = scale * dz, dgamma/dbeta unsupported
        if g_need or b_need:
            raise NotImplementedError('gradients of BatchNorm affine parameters in eval mode')
        coef = torch.zeros((3, kp), dtype=F32, device=g.device)
        coef[0] = n.scale
    if not need_dy:
        return None, None
    dy = torch.empty_like(n.y)
    event = n.region.raw_event() if side and form.carries_event else None
    ds_ptr, ds_acc = None, 0
    if sc is not None and sc.requires_grad:
        assert form.writes_shortcut
        # a gradient buffer this unit owns is masked in place and donated to a shortcut that has no gradient yet
        tgt, ds_acc = (g, 0) if n.out.grad_owned and donate_grad(sc, g) else grad_target(sc)
        ds_ptr = ptr(tgt)
    if event is not None:
        lib.tok_next_launch_event(event)      # armed right in front of the launch that carries it
    try:
        form.apply(lib, st, n, g, coef, dy, ds_ptr, ds_acc, m, kp)
    finally:
        if event is not None:
            lib.tok_next_launch_event(None)   # never left armed for an unrelated later launch
    return dy, event
