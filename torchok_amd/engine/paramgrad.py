"""How a unit's backward produces and commits parameter gradients: the one place a new unit gets its gradient sinks, its
weight-gradient / column-sum launches and its side-stream decision from.

A parameter's gradient lives in its fp32 slot (core.grad_slot).  `sink(p)` -> (slot, accumulate) is what a kernel needs;
`commit(p, slot, accumulate)` afterwards makes `p.grad` show the result and fires core.param_grad_hooks (the DDP bucket
launches hang on them: from here and nowhere else).  The three states of `p.grad`:
    None                   the kernel writes the slot (accumulate 0), commit points p.grad at it
    the slot               the kernel adds in the slot (accumulate 1), commit has nothing to move
    a tensor of the user   the kernel writes the slot (accumulate 0: the slot is free scratch then), commit adds it to p.grad
"""
import torch

from .. import _C
from . import core
from .core import grad_slot, ptr, stream_ptr

F32 = torch.float32


# ---- sinks -----------------------------------------------------------------------------------------------------------------
def sink(p: torch.nn.Parameter):
    slot = grad_slot(p)
    g = p.grad
    return slot, int(g is not None and g.data_ptr() == slot.data_ptr())


def commit(p: torch.nn.Parameter, slot: torch.Tensor, accumulate: int):
    if not accumulate:
        if p.grad is None:
            p.grad = slot
        else:
            p.grad.add_(slot)
    for h in core.param_grad_hooks:
        h(p)


def store(dst: torch.Tensor, accumulate: int, value: torch.Tensor):
    """dst (+)= value: a gradient that was computed elsewhere (another layout, a slice, a temporary) enters its sink."""
    if accumulate:
        dst.add_(value)
    else:
        dst.copy_(value)


def pair_sinks(p0, p1):
    """Sinks for a kernel that takes ONE accumulate flag for the gradients of two parameters (None: that one is frozen).
    -> (buffer 0, buffer 1, accumulate, finish).  Where the two flags agree the kernel writes the slots; where they do not,
    both results go through temporaries and `finish()` folds them in.  `finish()` commits either way."""
    s0 = sink(p0) if p0 is not None else None
    s1 = sink(p1) if p1 is not None else None
    if s0 is not None and s1 is not None and s0[1] != s1[1]:
        t0, t1 = torch.empty_like(s0[0]), torch.empty_like(s1[0])

        def finish():
            store(s0[0], s0[1], t0)
            commit(p0, *s0)
            store(s1[0], s1[1], t1)
            commit(p1, *s1)
        return t0, t1, 0, finish

    def finish():
        if s0 is not None:
            commit(p0, *s0)
        if s1 is not None:
            commit(p1, *s1)
    one = s0 if s0 is not None else s1
    return (s0[0] if s0 is not None else None, s1[0] if s1 is not None else None, one[1] if one is not None else 0, finish)


# ---- weight gradient of a GEMM-shaped layer ----------------------------------------------------------------------------------
_plans = {}


def wgrad_plan(d: _C.ConvDesc):
    """(the bias gradient can ride the weight-gradient kernel?, workspace bytes with it, without it) of a geometry: asked of
    the library once, not on every step on the launch thread."""
    lib = _C.lib()
    key = (bytes(d), id(lib))
    p = _plans.get(key)
    if p is None:
        p = _plans[key] = (bool(lib.tok_conv_wgrad_bias_ok(d)), int(lib.tok_conv_wgrad_bias_ws_bytes(d)),
                           int(lib.tok_conv_wgrad_ws_bytes(d)))
    return p


def weight_grad(d: _C.ConvDesc, x: torch.Tensor, dy: torch.Tensor, k: int, c: int, weight=None, out=None, accumulate=0,
                bias=None, bias_out=None):
    """dW[k][..][c] = dy^T x on the current stream -> (where it went, the workspace: keep it alive while the launch runs).
    weight: the parameter whose sink takes it (committed here); otherwise the plain fp32 buffer `out` (a new [k][c] one if
    None): a Gram matrix, a slice or another layout of a gradient the caller folds in itself, or a sink the caller commits.
    bias / bias_out: the column sums of dy ride the same launch (the caller has asked wgrad_plan), into the sink of that
    parameter (committed here) or into a plain fp32 vector (several sinks: the caller scatters it)."""
    lib = _C.lib()
    rides = bias is not None or bias_out is not None
    ws_bytes = wgrad_plan(d)[1 if rides else 2]
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=F32, device=x.device)
    if weight is not None:
        dst, acc = sink(weight)
    else:
        dst, acc = out if out is not None else torch.empty((k, c), dtype=F32, device=x.device), accumulate
    if rides:
        bdst, bacc = sink(bias) if bias is not None else (bias_out, 0)
        _C.check(lib.tok_conv_wgrad_bias(d, ptr(x), ptr(dy), ptr(dst), k, c, ptr(ws), ws_bytes, acc, ptr(bdst), bacc,
                                         stream_ptr()), 'tok_conv_wgrad_bias')
        if bias is not None:
            commit(bias, bdst, bacc)
    else:
        _C.check(lib.tok_conv_wgrad(d, ptr(x), ptr(dy), ptr(dst), k, c, ptr(ws), ws_bytes, acc, stream_ptr()),
                 'tok_conv_wgrad')
    if weight is not None:
        commit(weight, dst, acc)
    return dst, ws


# ---- bias gradient: column sums of dy ---------------------------------------------------------------------------------------
def colsum(dy: torch.Tensor, m: int, n_pad: int, dst: torch.Tensor, accumulate: int, two_pass: bool, n_real: int = 0):
    """dst (+)= column sums of the bf16 [m][n_pad] matrix dy.  two_pass: coalesced row-chunk partials, then a fixed-order fold
    (tall matrices; the partial rows are returned: keep them alive while the launches run); otherwise one tok_colsum launch
    over the first n_real columns.  Which one serves a layer is the caller's choice."""
    lib, st = _C.lib(), stream_ptr()
    if not two_pass:
        _C.check(lib.tok_colsum(ptr(dy), m, n_pad, n_real, ptr(dst), accumulate, st), 'tok_colsum')
        return None
    nrows = lib.tok_colsum_partial_rows(m, n_pad)
    part = torch.empty((nrows, n_pad), dtype=F32, device=dy.device)
    _C.check(lib.tok_colsum_partial(ptr(dy), m, n_pad, ptr(part), st), 'tok_colsum_partial')
    _C.check(lib.tok_colsum_f32(ptr(part), nrows, n_pad, ptr(dst), accumulate, st), 'tok_colsum_f32')
    return part


# ---- side stream: parameter gradients beside the main chain ------------------------------------------------------------------
# Nothing on the main chain waits for a parameter gradient.  Which units fork theirs (functional.py has the measurements):
CONV = 'conv'      # LDS/MFMA-bound or short-M weight gradients (functional._wgrad_side_ok), units of the main stream only
TOKEN = 'token'    # token layers and LayerNorm: always
NECK = 'neck'      # units of the main stream only (functional._side_for_tag)


def goes_side(node, g: torch.Tensor, policy: str, rows: int = 0) -> bool:
    """Do the parameter gradients of `node` (gradient tensor g; CONV: over `rows` output rows) run on the side stream?"""
    from . import functional as EF
    if not (EF.WGRAD_SIDE_STREAM and g.is_cuda and node.region is not None):
        return False
    if policy != TOKEN and not EF._side_for_tag(node.stream_tag, node.region):
        return False
    if policy == CONV:
        w = node.conv.weight
        r, s = (w.shape[2], w.shape[3]) if w.dim() == 4 else (1, 1)
        if not EF._wgrad_side_ok(r, s, rows, w.shape[0], w.shape[1]):
            return False
    return not torch.cuda.is_current_stream_capturing()      # nothing forks while a stream is being captured


def run_beside(node, side: bool, reads, fn, raw_event=None):
    """Run fn() — launches that produce parameter gradients only — on the side stream behind what the main stream has been
    given so far (side), or inline.  `reads` (what the launches read) and what fn returns (their scratch) stay referenced
    until the region joins the side stream."""
    if not side:
        fn()
        return
    with node.region.fork_side(reads, raw_event=raw_event):
        node.region.keep_until_join(*(fn() or ()))
