"""Gradient clipping over the arenas of a fused optimizer: ``torch.nn.utils.clip_grad_norm_`` / ``clip_grad_value_`` as
Lightning's ``clip_gradients`` applies them (``trainer.gradient_clip_val`` / ``gradient_clip_algorithm``, reference
``constructor/config_structure.py:161-162``), between the gradient exchange and ``optimizer.step()``.

The kernels (csrc/grad_clip.hip) walk a span table: one entry per parameter that has a gradient in this step, across all
arenas of the optimizer.  A slot whose ``.grad`` is None still holds an older step's values (``zero_grad`` does not clear the
arena), so a norm over the whole gradient buffer would be wrong; the table lists exactly the parameters torch would see.
It is cached on the device, keyed on ``arena_generation`` and the per-arena ``grad_flags()`` pattern (the key of the
optimizers' own run cache), and re-uploaded only when that pattern changes: a steady-state step makes no host-to-device
copy and no host read, so the calls can be recorded into a hipGraph (engine/graph.py).  The fp64 partials and the
norm / coefficient scalars are allocated once per optimizer, at fixed addresses."""
import math
from typing import Optional, Tuple

import torch

from .. import _C
from ..engine.core import ptr, stream_ptr


def _arena_optimizer(optimizer, fn: str):
    from .optimizers import _ArenaOptimizer
    if not isinstance(optimizer, _ArenaOptimizer):
        raise TypeError(f'torchok_amd.optim.{fn} takes a fused arena optimizer (its gradients live in the arenas); for a plain '
                        f'iterable of parameters use torch.nn.utils.{fn}')
    optimizer._ensure_built()
    return optimizer


class _ClipState:
    """Per optimizer: the device span table of the current gradient pattern, and the workspace of the norm."""

    def __init__(self, device):
        self.key = None
        self.table: Optional[torch.Tensor] = None       # int64 [n, 3]: tok_grad_span (grad pointer, numel, start)
        self.n = 0
        self.total = 0
        self.device = device
        self.partials = torch.empty(_C.TOK_GRAD_CLIP_MAX_PARTIALS, dtype=torch.float64, device=device)
        self.scalars = torch.zeros(2, dtype=torch.float32, device=device)    # [total norm, clip coefficient]


def _spans(optimizer) -> Optional[_ClipState]:
    """The clip state with a span table for the gradients present now (foreign .grad tensors adopted into their slots first,
    as the optimizer step does); None when the optimizer has no parameters at all."""
    arenas = [a for a in optimizer._arenas if a is not None]
    if not arenas:
        return None
    st = getattr(optimizer, '_clip_state', None)
    if st is None or st.device != arenas[0].grad.device:
        st = optimizer._clip_state = _ClipState(arenas[0].grad.device)
    flags = [a.adopt_grads() for a in arenas]
    key = (optimizer.arena_generation, [list(map(bool, fl)) for fl in flags])     # presence only: 1 and 2 are one slot
    if key != st.key:
        rows, start = [], 0
        for a, fl in zip(arenas, flags):
            base = a.grad.data_ptr()
            for i, f in enumerate(fl):
                n = a.params[i].numel()
                if f and n:
                    rows.append((base + 4 * a.offsets[i], n, start))
                    start += n
        st.table = torch.tensor(rows, dtype=torch.int64).to(st.device) if rows else None
        st.n, st.total, st.key = len(rows), start, key
    return st


def _clip_norm(optimizer, max_norm: float, error_if_nonfinite: bool = False) -> torch.Tensor:
    """clip_grad_norm_ without the copy of the result: the returned 0-dim tensor is the optimizer's norm scalar, rewritten by
    the next call.  Three launches: per-block fp64 partials, the fixed-order fold into norm and coefficient, the scale."""
    if error_if_nonfinite and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError('clip_grad_norm_(error_if_nonfinite=True) reads the norm on the host: not inside a graph capture')
    st = _spans(optimizer)
    if st is None or st.n == 0:
        return torch.zeros((), dtype=torch.float32, device=st.device if st is not None else None)
    lib, s = _C.lib(), stream_ptr()
    tbl, norm, coef = ptr(st.table), ptr(st.scalars), ptr(st.scalars) + 4
    _C.check(lib.tok_grad_sqnorm_partial(tbl, st.n, st.total, ptr(st.partials), s), 'tok_grad_sqnorm_partial')
    _C.check(lib.tok_grad_clip_coef(ptr(st.partials), st.total, float(max_norm), norm, coef, s), 'tok_grad_clip_coef')
    if error_if_nonfinite:
        total = float(st.scalars[0])
        if not math.isfinite(total):
            raise RuntimeError('The total norm of order 2.0 for gradients from `parameters` is non-finite, so it cannot be '
                               'clipped. To disable this error and scale the gradients by the non-finite norm anyway, set '
                               '`error_if_nonfinite=False`')
    _C.check(lib.tok_grad_scale(tbl, st.n, st.total, coef, s), 'tok_grad_scale')
    return st.scalars[0]


@torch.no_grad()
def clip_grad_norm_(optimizer, max_norm: float, norm_type: float = 2.0, error_if_nonfinite: bool = False,
                    foreach=None) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ over the gradients of a fused arena optimizer's parameters (those whose .grad is not
    None).  Returns the total norm as a 0-dim fp32 device tensor, without a host read (unless error_if_nonfinite, which reads
    it and raises like torch; refused inside a graph capture).  Only norm_type 2 (the one Lightning's trainer uses).
    `foreach` is accepted for signature compatibility and ignored."""
    _arena_optimizer(optimizer, 'clip_grad_norm_')
    if float(norm_type) != 2.0:
        raise NotImplementedError(f'clip_grad_norm_: norm_type={norm_type!r}; only the 2-norm is built')
    return _clip_norm(optimizer, float(max_norm), error_if_nonfinite).clone()


@torch.no_grad()
def clip_grad_value_(optimizer, clip_value: float, foreach=None) -> None:
    """torch.nn.utils.clip_grad_value_ over the gradients of a fused arena optimizer's parameters: every gradient element is
    clamped to [-clip_value, clip_value] in place, NaN preserved.  One launch."""
    _arena_optimizer(optimizer, 'clip_grad_value_')
    st = _spans(optimizer)
    if st is None or st.n == 0:
        return
    _C.check(_C.lib().tok_grad_clamp(ptr(st.table), st.n, st.total, float(clip_value), stream_ptr()), 'tok_grad_clamp')


def clip_gradients(optimizer, clip: Tuple[str, float]) -> None:
    """What Lightning's `clip_gradients` does with (gradient_clip_algorithm, gradient_clip_val): ('norm', max_norm) or
    ('value', clip_value).  run.resolve_gradient_clip turns a trainer config into this pair (or None: no clipping)."""
    algo, val = clip
    if algo == 'norm':
        _clip_norm(_arena_optimizer(optimizer, 'clip_grad_norm_'), float(val))
    elif algo == 'value':
        clip_grad_value_(optimizer, float(val))
    else:
        raise ValueError(f'gradient clipping algorithm {algo!r}: "norm" or "value"')
