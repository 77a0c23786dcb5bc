"""Engine units of the token-major (SwinV2) rows.  Tokens are rows of a bf16 [B*H*W][C] matrix.

Unit                 replaces ([timm 0.6.13] swin_transformer_v2 through torchok/models/backbones/swin.py)
-------------------  -------------------------------------------------------------------------------------
linear_op            F.linear (qkv with cat(q_bias, k_bias, v_bias); proj; Mlp.fc1/fc2; PatchMerging.reduction;
                     cpb_mlp) on the MFMA conv kernels (1x1, h = w = 1)
layer_norm           nn.LayerNorm, optionally fused with the res-post-norm residual  x + drop_path(norm(.))
activation           GELU (Mlp) / ReLU (cpb_mlp)
cpb_bias             16 * sigmoid(cpb_mlp(relative_coords_table))[relative_position_index]
window_attention     WindowAttention.forward between qkv and proj, with roll / window_partition / window_reverse
                     folded into the kernel's token addressing
patch_merge          PatchMerging's strided 2x2 gather + cat
reshape              .view between (B, H, W, C) maps and (B*H*W, C) token rows (zero copy)
global_attention     ViT Attention.forward between qkv and proj: softmax(q k^T / 8) v over all tokens of an image; with
                     `bias` BEiT's softmax(q k^T / 8 + relative_position_bias) v
relpos_bias          BEiT relative_position_bias_table[relative_position_index] -> [heads][N][N] (gathered again in the backward)
gc_window_attention  GCViT WindowAttentionGlobal.forward between qkv and proj: softmax(q k^T / sqrt(32) + bias) v per window, the
                     query from the tokens or from the stage's shared q_global map
layer_scale_add      BEiT Block's  x + drop_path(gamma * f(x))
patch_embed          ViT PatchEmbed.proj (k = stride = patch): patch gather + 1x1 GEMM
vit_embed            VisionTransformer._pos_embed: cls token + pos_embed, one rounding
rows_select          x[:, first:first + count] of the (B, T, C) token view (cls rows, patch rows)
"""
import os
from typing import List, Optional, Sequence, Tuple

import torch
from torch import nn

from .. import _C
from . import paramgrad as PG
from .core import BF16, Node, Region, TTensor, await_mark, await_ready, donate_grad, grad_target, pad8, ptr, stream_ptr, written_mark
from .functional import _krsc, get_packs

F32 = torch.float32


def _rows(t: TTensor) -> int:
    return t.data.numel() // t.data.shape[-1]


# ---- reshape (zero copy) --------------------------------------------------------------------------------
class _ReshapeNode(Node):
    needs_backward = True

    def backward(self):
        g = self.out.grad
        if g is None or not self.x.requires_grad:
            return
        gv = g.view(self.x.data.shape)
        if not donate_grad(self.x, gv):
            tgt, _ = grad_target(self.x)
            _C.check(_C.lib().tok_act_bwd(2, ptr(gv), ptr(gv), ptr(tgt), 1, gv.numel(), stream_ptr()), 'tok_act_bwd')
        self.out.grad = None

    def release(self):
        self.x = self.out = None


def reshape(region: Region, x: TTensor, shape: Sequence[int]) -> TTensor:
    out = TTensor(x.data.view(*shape), x.c, requires_grad=x.requires_grad and region.grad_mode)
    if out.requires_grad:
        node = _ReshapeNode()
        node.x, node.out = x, out
        out.node = node
        x.uses += 1
        region.add(node)
    return out


# ---- linear --------------------------------------------------------------------------------------------------
class _LinearNode(Node):
    needs_backward = True
    mlp_first = None        # fc2 of a fused Mlp: the node of its fc1 (tok_mlp_bwd_dx covers both data gradients)
    dx_done = False         # fc1 of a fused Mlp: its data gradient was produced by fc2's backward launch

    def backward(self):
        lib, st = _C.lib(), stream_ptr()
        g = self.out.grad
        if g is None:
            return
        x, w, d = self.x, self.weight, self.desc
        m, kp = g.shape
        side = PG.goes_side(self, g, PG.TOKEN)
        sinks = [(p, start) for p, start in self.bias_sinks if p.requires_grad]

        def scatter_bias(tmp):
            for p, start in sinks:
                slot, acc = PG.sink(p)
                PG.store(slot, acc, tmp[start:start + p.numel()])
                PG.commit(p, slot, acc)
        # the column sums of g (bias gradients) come out of the weight-gradient kernel where it serves the layer; the
        # parameter gradients are enqueued before the data gradient (the other order measured neutral: SwinV2-T 24.98 vs
        # 24.97, DaViT-T 24.33 vs 24.20 ms/step), off the main chain and beside it (PG.TOKEN)
        bias_in_wgrad = bool(self.bias_sinks and w.requires_grad and PG.wgrad_plan(d)[0])
        if self.bias_sinks and not bias_in_wgrad:
            def run_bias():
                tmp = torch.empty(kp, dtype=F32, device=g.device)
                part = PG.colsum(g, m, kp, tmp, 0, two_pass=True)
                scatter_bias(tmp)
                return tmp, part
            PG.run_beside(self, side, (g,), run_bias)
        if w.requires_grad:
            k, _, _, c = _krsc(w)

            def run_wgrad():
                if not bias_in_wgrad:
                    return PG.weight_grad(d, x.data, g, k, c, weight=w)[1:]
                if len(self.bias_sinks) == 1 and len(sinks) == 1 and sinks[0][1] == 0 and sinks[0][0].numel() == k:
                    # one bias parameter spanning all output features (fc1 / fc2 / proj): the kernel writes its sink itself
                    return PG.weight_grad(d, x.data, g, k, c, weight=w, bias=sinks[0][0])[1:]
                slot, acc = PG.sink(w)
                tmp = torch.empty(kp, dtype=F32, device=g.device)
                ws = PG.weight_grad(d, x.data, g, k, c, out=slot, accumulate=acc, bias_out=tmp)[1]
                scatter_bias(tmp)
                PG.commit(w, slot, acc)
                return (ws,)
            PG.run_beside(self, side, (x.data, g), run_wgrad)
        if x.requires_grad and self.dx_done:
            pass            # fc1 of a fused Mlp: fc2's backward launch already sent this gradient on (tok_mlp_bwd_dx)
        elif x.requires_grad:
            an = x.node
            first = self.mlp_first
            if (FUSE_ACT and isinstance(an, _ActNode) and an.out is x and an.kind in (RELU, GELU) and x.uses == 1 and
                    x.grad is None and an.x.requires_grad and an.x.uses == 1 and an.x.grad is None):
                if (first is not None and FUSE_MLP_BWD and an.kind == GELU and an.x is first.out and first.x.requires_grad
                        and first.pk.dgrad is not None):
                    # fc2 of a fused Mlp: d(pre) = (dy W2) * GELU'(pre) stays in registers and goes straight through W1 to the
                    # Mlp's input; the d(pre) rows are written only if fc1's parameter gradients will read them
                    w1, sinks = first.weight, first.bias_sinks
                    need_dpre = w1.requires_grad or any(p.requires_grad for p, _ in sinks)
                    tgt = grad_target(an.x)[0] if need_dpre else None
                    tgt_x, acc_x = grad_target(first.x)
                    _C.check(lib.tok_mlp_bwd_dx(ptr(g), ptr(self.pk.dgrad), ptr(an.x.data), ptr(first.pk.dgrad), ptr(tgt_x), acc_x,
                                                ptr(tgt), m, d.k, d.c, st), 'tok_mlp_bwd_dx')
                    first.dx_done = True
                else:
                    # this layer consumes act(h) and nothing else does: its dgrad epilogue multiplies by act'(h) and writes
                    # d(h) — the gradient of act(h) is never materialised, the activation node finds nothing to do
                    tgt, _ = grad_target(an.x)
                    _C.check(lib.tok_conv_dgrad_act(d, ptr(g), ptr(self.pk.dgrad), ptr(an.x.data), an.kind, ptr(tgt), st),
                             'tok_conv_dgrad_act')
            else:
                tgt, acc = grad_target(x)
                _C.check(lib.tok_conv_dgrad(d, ptr(g), ptr(self.pk.dgrad), ptr(tgt), acc, st), 'tok_conv_dgrad')
        self.out.grad = None

    def release(self):
        self.x = self.out = self.pk = self.mlp_first = None


# GELU / ReLU in the epilogues of the GEMMs around it (tok_conv_fwd_act / tok_conv_dgrad_act).  Bit-identical to the separate
# launches.  Round 2 measured it NEUTRAL with libm's erff / expf (SwinV2-T B=256: 29.0 vs 29.0 ms/step — ~55 VALU per element
# stretched the epilogue by what the deleted passes cost); with the 14-instruction erf of tok_common.h (round 3) the fused form
# wins: SwinV2-T 24.87 -> 24.59, DaViT-T 24.14 -> 23.95 ms/step, and 12 activation-sized tensor passes per block leave the
# step's HBM traffic.  On by default; TOK_FUSE_ACT=0 restores the separate launches.
FUSE_ACT = os.environ.get('TOK_FUSE_ACT', '1') == '1'


def linear_op(region: Region, x: TTensor, weight: nn.Parameter, bias_vec: Optional[torch.Tensor] = None,
              bias_sinks: Sequence[Tuple[nn.Parameter, int]] = (), act: Optional[int] = None):
    """y = x W^T + bias_vec.  `bias_vec` is an fp32 vector of the (padded) output width; `bias_sinks` lists the
    parameters it was assembled from as (param, start column) — their gradients are column sums of dy.
    act = RELU / GELU: returns act(y) instead, produced by the same launch (y is kept for the backward)."""
    lib, st = _C.lib(), stream_ptr()
    k, c = weight.shape
    n, cp = x.shape
    if pad8(c) != cp:
        raise ValueError(f'linear_op: input width {cp} does not match in_features {c}')
    kp = pad8(k)
    need_dx = region.grad_mode and x.requires_grad
    pk = get_packs(weight, None, kp, 1, cp, want_dgrad=need_dx, refresh=True)
    if bias_vec is not None and bias_vec.shape[0] != kp:
        b = torch.zeros(kp, dtype=F32, device=bias_vec.device)
        b[:bias_vec.shape[0]] = bias_vec
        bias_vec = b
    d = _C.ConvDesc(n, 1, 1, cp, kp, 1, 1, 1, 1, 1, 0, 1)
    y = torch.empty((n, kp), dtype=BF16, device=x.data.device)
    y_act = None
    if act is not None and FUSE_ACT:
        y_act = torch.empty_like(y)
        _C.check(lib.tok_conv_fwd_act(d, ptr(x.data), ptr(pk.fwd), ptr(bias_vec), ptr(y), ptr(y_act), act, st),
                 'tok_conv_fwd_act')
    else:
        _C.check(lib.tok_conv_fwd(d, ptr(x.data), ptr(pk.fwd), ptr(bias_vec), ptr(y), None, st), 'tok_conv_fwd')
    out = _record_linear(region, x, weight, bias_sinks, y, d, pk)
    if act is None:
        return out
    return activation(region, out, act, precomputed=y_act)


def _record_linear(region: Region, x: TTensor, weight: nn.Parameter, bias_sinks, y: torch.Tensor, d, pk) -> TTensor:
    """The tape entry of y = x W^T + b, whoever launched it."""
    k = weight.shape[0]
    req = region.grad_mode and (x.requires_grad or weight.requires_grad or any(p.requires_grad for p, _ in bias_sinks))
    out = TTensor(y, k, requires_grad=req)
    if req:
        node = _LinearNode()
        node.x, node.out, node.weight, node.desc, node.pk = x, out, weight, d, pk
        node.bias_sinks = list(bias_sinks)
        out.node = node
        if x.requires_grad:
            x.uses += 1
        region.add(node)
    return out


def linear_module(region: Region, x: TTensor, fc: nn.Linear, act: Optional[int] = None) -> TTensor:
    if fc.bias is None:
        return linear_op(region, x, fc.weight, act=act)
    return linear_op(region, x, fc.weight, fc.bias.detach(), [(fc.bias, 0)], act=act)


# The whole Mlp from one launch (csrc/mlp_fused.hip): fc2 consumes GELU(fc1(x)) out of registers; in training the bf16
# pre-activation and activation rows are still written (the backward GEMMs read them), so the tape is the one the separate
# launches record and every tensor on it has the same bits.  Measured per call on the SwinV2-T B=256 shapes (fused+saved vs
# fc1+GELU launch + fc2 launch): C=96 366 vs 543 us, C=192 269 vs 368, C=384 203 vs 239.  TOK_FUSE_MLP=0: separate launches.
FUSE_MLP = os.environ.get('TOK_FUSE_MLP', '1') == '1'
# ... and its backward to the input from one launch too (tok_mlp_bwd_dx replaces tok_conv_dgrad_act + tok_conv_dgrad; the d(pre)
# rows are still written for fc1's weight gradient).  Per call: C=96 360 vs 600 us, C=192 267 vs 373, C=384 216 vs 242.
FUSE_MLP_BWD = os.environ.get('TOK_FUSE_MLP_BWD', '1') == '1'


def mlp_module(region: Region, x: TTensor, fc1: nn.Linear, fc2: nn.Linear) -> TTensor:
    """fc2(GELU(fc1(x))) — [timm 0.6.13] models/layers/mlp.py: Mlp.forward with drop = 0."""
    lib = _C.lib()
    n, cp = x.shape
    c, hid = fc1.in_features, fc1.out_features
    served = (FUSE_MLP and FUSE_ACT and fc1.bias is not None and fc2.bias is not None and cp == c
              and fc2.in_features == hid and fc2.out_features == c and bool(lib.tok_mlp_serves(n, c, hid)))
    if not served:
        h = linear_module(region, x, fc1, act=GELU)      # fc1 + GELU: one launch; fc2's dgrad applies GELU'
        return linear_module(region, h, fc2)
    st = stream_ptr()
    params = (fc1.weight, fc1.bias, fc2.weight, fc2.bias)
    train = region.grad_mode and (x.requires_grad or any(p.requires_grad for p in params))
    pk1 = get_packs(fc1.weight, None, hid, 1, cp, want_dgrad=region.grad_mode and x.requires_grad, refresh=True)
    pk2 = get_packs(fc2.weight, None, c, 1, hid, want_dgrad=train, refresh=True)
    dev = x.data.device
    y = torch.empty((n, c), dtype=BF16, device=dev)
    pre = act = None
    if train:
        pre = torch.empty((n, hid), dtype=BF16, device=dev)
        act = torch.empty_like(pre)
    _C.check(lib.tok_mlp_fwd(ptr(x.data), ptr(pk1.fwd), ptr(fc1.bias.detach()), ptr(pk2.fwd), ptr(fc2.bias.detach()), ptr(y),
                             ptr(pre), ptr(act), n, c, hid, st), 'tok_mlp_fwd')
    if not train:
        return TTensor(y, c, requires_grad=False)
    d1 = _C.ConvDesc(n, 1, 1, cp, hid, 1, 1, 1, 1, 1, 0, 1)
    d2 = _C.ConvDesc(n, 1, 1, hid, c, 1, 1, 1, 1, 1, 0, 1)
    h_pre = _record_linear(region, x, fc1.weight, [(fc1.bias, 0)], pre, d1, pk1)
    h = activation(region, h_pre, GELU, precomputed=act)
    out = _record_linear(region, h, fc2.weight, [(fc2.bias, 0)], y, d2, pk2)
    if out.node is not None and h_pre.node is not None:
        out.node.mlp_first = h_pre.node
    return out


# ---- layer norm (+ residual, + stochastic depth) ---------------------------------------------------------------------
class _LayerNormNode(Node):
    needs_backward = True

    def backward(self):
        lib, st = _C.lib(), stream_ptr()
        g = self.out.grad
        if g is None:
            return
        x, ln, sc = self.x, self.ln, self.shortcut
        rows, cp = _rows(x), x.cp
        c = x.c
        need_param = ln.weight.requires_grad or ln.bias.requires_grad
        if x.requires_grad or need_param:
            nrows = lib.tok_layernorm_bwd_rows(rows, c)
            partial = torch.empty((2, nrows, c), dtype=F32, device=g.device)
            if x.requires_grad:
                tgt, acc = grad_target(x)
            else:
                tgt, acc = torch.empty_like(x.data), 0
            _C.check(lib.tok_layernorm_bwd(ptr(g), ptr(x.data), ptr(self.mean), ptr(self.rstd), ptr(ln.weight),
                                           ptr(self.row_scale), self.rps, ptr(tgt), acc, ptr(partial), rows, c, cp, st),
                     'tok_layernorm_bwd')
            def run_param_grads():
                st_ = stream_ptr()
                (sw, aw), (sb, ab) = (PG.sink(p) if p.requires_grad else (None, 0) for p in (ln.weight, ln.bias))
                if sw is not None and sb is not None:        # both folds in one launch
                    _C.check(lib.tok_colsum_f32_pair(ptr(partial[0]), ptr(partial[1]), nrows, c, ptr(sw), aw, ptr(sb), ab, st_),
                             'tok_colsum_f32_pair')
                else:
                    for slot, acc, part in ((sw, aw, partial[0]), (sb, ab, partial[1])):
                        if slot is not None:
                            _C.check(lib.tok_colsum_f32(ptr(part), nrows, c, ptr(slot), acc, st_), 'tok_colsum_f32')
                for p, slot, acc in ((ln.weight, sw, aw), (ln.bias, sb, ab)):
                    if slot is not None:
                        PG.commit(p, slot, acc)
            PG.run_beside(self, PG.goes_side(self, g, PG.TOKEN), (partial,), run_param_grads)
        if sc is not None and sc.requires_grad:
            # the residual branch passes the gradient through: hand the buffer over when we own it
            if not (self.out.grad_owned and donate_grad(sc, g.view(sc.data.shape))):
                tgt, acc = grad_target(sc)
                _C.check(lib.tok_act_bwd(2, ptr(g), ptr(g), ptr(tgt), acc, g.numel(), st), 'tok_act_bwd')
        self.out.grad = None

    def release(self):
        self.x = self.out = self.shortcut = self.mean = self.rstd = self.row_scale = None


def layer_norm(region: Region, x: TTensor, ln: nn.LayerNorm, shortcut: Optional[TTensor] = None,
               row_scale: Optional[torch.Tensor] = None, rows_per_sample: int = 0) -> TTensor:
    """out = shortcut + row_scale[sample] * LayerNorm(x)."""
    if ln.weight is None or ln.bias is None or len(ln.normalized_shape) != 1 or ln.normalized_shape[0] != x.c:
        raise NotImplementedError('layer_norm: affine LayerNorm over the channel dimension only')
    lib, st = _C.lib(), stream_ptr()
    rows, cp = _rows(x), x.cp
    dev = x.data.device
    out_data = torch.empty_like(x.data)
    mean = torch.empty(rows, dtype=F32, device=dev)
    rstd = torch.empty(rows, dtype=F32, device=dev)
    _C.check(lib.tok_layernorm_fwd(ptr(x.data), ptr(shortcut.data) if shortcut is not None else None, ptr(row_scale),
                                   rows_per_sample, ptr(ln.weight), ptr(ln.bias), ptr(out_data), ptr(mean), ptr(rstd),
                                   rows, x.c, cp, float(ln.eps), st), 'tok_layernorm_fwd')
    req = region.grad_mode and (x.requires_grad or ln.weight.requires_grad or ln.bias.requires_grad or
                                (shortcut is not None and shortcut.requires_grad))
    out = TTensor(out_data, x.c, requires_grad=req)
    if req:
        node = _LayerNormNode()
        node.x, node.out, node.ln, node.shortcut = x, out, ln, shortcut
        node.mean, node.rstd, node.row_scale, node.rps = mean, rstd, row_scale, rows_per_sample
        out.node = node
        if x.requires_grad:
            x.uses += 1
        if shortcut is not None and shortcut.requires_grad:
            shortcut.uses += 1
        region.add(node)
    return out


# ---- activations ----------------------------------------------------------------------------------------------------------
RELU, GELU = 0, 1


class _ActNode(Node):
    needs_backward = True

    def backward(self):
        g = self.out.grad
        if g is None or not self.x.requires_grad:
            return
        tgt, acc = grad_target(self.x)
        _C.check(_C.lib().tok_act_bwd(self.kind, ptr(g), ptr(self.x.data), ptr(tgt), acc, g.numel(), stream_ptr()),
                 'tok_act_bwd')
        self.out.grad = None

    def release(self):
        self.x = self.out = None


def activation(region: Region, x: TTensor, kind: int, precomputed: Optional[torch.Tensor] = None) -> TTensor:
    """act(x); `precomputed` = act(x) already produced by the epilogue of the GEMM that made x."""
    if precomputed is not None:
        y = precomputed
    else:
        y = torch.empty_like(x.data)
        _C.check(_C.lib().tok_act_fwd(kind, ptr(x.data), ptr(y), y.numel(), stream_ptr()), 'tok_act_fwd')
    req = region.grad_mode and x.requires_grad
    out = TTensor(y, x.c, requires_grad=req)
    if req:
        node = _ActNode()
        node.x, node.out, node.kind = x, out, kind
        out.node = node
        x.uses += 1
        region.add(node)
    return out


# ---- continuous relative position bias ------------------------------------------------------------------------------------
class _CpbBiasNode(Node):
    """Backward of the position-bias unit.  The attention unit that consumed the bias leaves its per-workgroup partial
    rows of d(logits) and d(logit_scale) here (`scratch`, `dscale`, `mark`); their fixed-order folds, d(logit_scale) and
    the gather back onto the cpb_mlp output run on THIS unit's stream — a branch stream in SwinV2 (swin.py), so the
    dependent chain of the main stream carries none of these small launches."""
    needs_backward = True

    def backward(self):
        if self.scratch is None:
            return
        lib, st = _C.lib(), stream_ptr()
        await_mark(self.mark)
        rows, heads, n = self.scratch.shape[0], self.heads, self.n
        dev = self.scratch.device
        ls = self.logit_scale
        if ls is not None and ls.requires_grad:
            slot, acc = PG.sink(ls)
            _C.check(lib.tok_colsum_f32(ptr(self.dscale), rows, heads, ptr(slot), acc, st), 'tok_colsum_f32')
            PG.commit(ls, slot, acc)
        if not self.table.requires_grad:
            return
        dbias = torch.empty(heads * n * n, dtype=F32, device=dev)
        _C.check(lib.tok_colsum_f32(ptr(self.scratch), rows, heads * n * n, ptr(dbias), 0, st), 'tok_colsum_f32')
        trows, ld = self.table.shape
        tgt, acc = grad_target(self.table)
        if acc:
            raise RuntimeError('cpb_bias: the cpb_mlp output has a single consumer')
        _C.check(lib.tok_cpb_bias_bwd(ptr(dbias), 0, ptr(self.table.data), ld, ptr(self.index), heads, n, trows, ptr(tgt), st),
                 'tok_cpb_bias_bwd')

    def release(self):
        self.table = self.index = self.bias = self.scratch = self.dscale = self.mark = self.logit_scale = None


def cpb_bias(region: Region, table: TTensor, index: torch.Tensor, heads: int, n_tokens: int):
    """(bias fp32 [heads][N][N], node).  The attention unit hands its d(logits) / d(logit_scale) partial rows back through
    the node (see _CpbBiasNode)."""
    rows, ld = table.shape
    bias = torch.empty((heads, n_tokens, n_tokens), dtype=F32, device=table.data.device)
    _C.check(_C.lib().tok_cpb_bias_fwd(ptr(table.data), ld, ptr(index), heads, n_tokens, ptr(bias), stream_ptr()),
             'tok_cpb_bias_fwd')
    node = None
    if region.grad_mode and table.requires_grad:
        node = _CpbBiasNode()
        node.table, node.index, node.heads, node.n, node.bias = table, index, heads, n_tokens, bias
        node.scratch = node.dscale = node.mark = node.logit_scale = None
        table.uses += 1
        region.add(node)
    return bias, node


# ---- window attention ---------------------------------------------------------------------------------------------------------
class _WindowAttnNode(Node):
    needs_backward = True

    def backward(self):
        lib, st = _C.lib(), stream_ptr()
        g = self.out.grad
        if g is None:
            return
        b, h, w, c, heads, ws, shift = self.geo
        n = ws * ws
        nw = (h // ws) * (w // ws)
        qkv = self.qkv
        dev = g.device
        tgt, acc = grad_target(qkv)
        if acc:
            raise RuntimeError('window_attention: qkv has a single consumer')
        if self.logit_scale is None:       # plain scaled-dot-product windows (DaViT): no bias / scale gradients
            _C.check(lib.tok_window_attn_bwd(ptr(qkv.data), ptr(g), b, h, w, c, heads, ws, shift, qkv.cp, None, None, None,
                                             ptr(self.lse), ptr(tgt), None, None, st), 'tok_window_attn_bwd')
            if qkv.cp != 3 * c:
                tgt[:, 3 * c:] = 0
            self.out.grad = None
            return
        rows = lib.tok_window_attn_bwd_rows(b, h, w, heads, ws)
        scratch = torch.empty((rows, heads * n * n), dtype=F32, device=dev)
        dscale = torch.empty((rows, heads), dtype=F32, device=dev)
        _C.check(lib.tok_window_attn_bwd(ptr(qkv.data), ptr(g), b, h, w, c, heads, ws, shift, qkv.cp,
                                         ptr(self.logit_scale), ptr(self.bias), ptr(self.mask), ptr(self.lse), ptr(tgt),
                                         ptr(scratch), ptr(dscale), st), 'tok_window_attn_bwd')
        if qkv.cp != 3 * c:
            tgt[:, 3 * c:] = 0
        ls = self.logit_scale
        bn = self.bias_node
        if bn is not None:
            # folds and parameter gradients happen in the position-bias unit's backward (its own stream)
            bn.scratch, bn.dscale, bn.logit_scale, bn.mark = scratch, dscale, ls, written_mark()
        elif ls.requires_grad:
            slot, acc = PG.sink(ls)
            _C.check(lib.tok_colsum_f32(ptr(dscale), rows, heads, ptr(slot), acc, st), 'tok_colsum_f32')
            PG.commit(ls, slot, acc)
        self.out.grad = None

    def release(self):
        self.qkv = self.out = self.bias = self.mask = self.lse = self.bias_node = None


def window_attention(region: Region, qkv: TTensor, geo: Tuple[int, int, int, int, int, int, int],
                     logit_scale: Optional[nn.Parameter] = None, bias: Optional[torch.Tensor] = None, bias_node=None,
                     mask: Optional[torch.Tensor] = None) -> TTensor:
    """qkv rows [B*H*W][3C] -> attention output rows [B*H*W][C]; geo = (B, H, W, C, heads, window, shift).
    logit_scale / bias given: SwinV2 cosine attention; both None: softmax(q k^T / sqrt(head_dim)) v (DaViT)."""
    b, h, w, c, heads, ws, shift = geo
    if c != heads * 32:
        raise NotImplementedError('window_attention: head_dim 32 (every SwinV2 / DaViT variant of the reference)')
    if (logit_scale is None) != (bias is None):
        raise ValueError('window_attention: logit_scale and bias go together')
    lib, st = _C.lib(), stream_ptr()
    n = ws * ws
    nw = (h // ws) * (w // ws)
    dev = qkv.data.device
    out_data = torch.empty((b * h * w, c), dtype=BF16, device=dev)
    lse = torch.empty(b * nw * heads * n, dtype=F32, device=dev)
    _C.check(lib.tok_window_attn_fwd(ptr(qkv.data), b, h, w, c, heads, ws, shift, qkv.cp, ptr(logit_scale), ptr(bias),
                                     ptr(mask), ptr(out_data), ptr(lse), st), 'tok_window_attn_fwd')
    req = region.grad_mode and (qkv.requires_grad or (logit_scale is not None and logit_scale.requires_grad) or
                                bias_node is not None)
    out = TTensor(out_data, c, requires_grad=req)
    if req:
        node = _WindowAttnNode()
        node.qkv, node.out, node.geo, node.logit_scale = qkv, out, geo, logit_scale
        node.bias, node.bias_node, node.mask, node.lse = bias, bias_node, mask, lse
        out.node = node
        qkv.uses += 1
        region.add(node)
    return out


# ---- patch merging gather ----------------------------------------------------------------------------------------------------------
class _PatchMergeNode(Node):
    needs_backward = True

    def backward(self):
        g = self.out.grad
        if g is None or not self.x.requires_grad:
            return
        b, h, w, c = self.geo
        tgt, acc = grad_target(self.x)
        lib, st = _C.lib(), stream_ptr()
        if acc:      # the stage output also feeds its feature norm (forward_features): un-permute, then add
            tmp = torch.empty_like(tgt)
            _C.check(lib.tok_patch_merge(ptr(g), ptr(tmp), b, h, w, c, 1, st), 'tok_patch_merge')
            _C.check(lib.tok_act_bwd(2, ptr(tmp), ptr(tmp), ptr(tgt), 1, tmp.numel(), st), 'tok_act_bwd')
        else:
            _C.check(lib.tok_patch_merge(ptr(g), ptr(tgt), b, h, w, c, 1, st), 'tok_patch_merge')
        self.out.grad = None

    def release(self):
        self.x = self.out = None


def patch_merge(region: Region, x: TTensor, b: int, h: int, w: int) -> TTensor:
    """token rows [B*H*W][C] -> [B*(H/2)*(W/2)][4C] (x0, x1, x2, x3 concatenation of PatchMerging)."""
    c = x.c
    if c != x.cp:
        raise NotImplementedError('patch_merge: channels % 8 == 0')
    y = torch.empty((b * (h // 2) * (w // 2), 4 * c), dtype=BF16, device=x.data.device)
    _C.check(_C.lib().tok_patch_merge(ptr(x.data), ptr(y), b, h, w, c, 0, stream_ptr()), 'tok_patch_merge')
    req = region.grad_mode and x.requires_grad
    out = TTensor(y, 4 * c, requires_grad=req)
    if req:
        node = _PatchMergeNode()
        node.x, node.out, node.geo = x, out, (b, h, w, c)
        out.node = node
        x.uses += 1
        region.add(node)
    return out


# ---- DaViT: channel attention and the pre-norm residual ------------------------------------------------------------------------
class _ChannelAttnNode(Node):
    needs_backward = True

    def backward(self):
        lib, st = _C.lib(), stream_ptr()
        g = self.out.grad
        if g is None or not self.qkv.requires_grad:
            return
        images, rpi, heads, c, scale = self.geo
        qkv, ld = self.qkv, self.qkv.cp
        q, k, v = (ptr(qkv.data) + 2 * o for o in (0, c, 2 * c))
        tgt, acc = grad_target(qkv)
        if acc:
            raise RuntimeError('channel_attention: qkv has a single consumer')
        dq, dk, dv = (ptr(tgt) + 2 * o for o in (0, c, 2 * c))
        ds = torch.empty_like(self.attn)
        # dA = dout^T q, through the softmax: dS = A o (dA - rowsum(dA o A))
        _C.check(lib.tok_chan_gram(ptr(g), g.stride(0), q, ld, rpi, images, heads, 1.0, 2, ptr(self.attn), ptr(ds), st),
                 'tok_chan_gram')
        _C.check(lib.tok_chan_apply(ptr(g), g.stride(0), ptr(self.attn), 1, 1.0, rpi, images, heads, dq, ld, st),
                 'tok_chan_apply')                                   # dq = dout A
        _C.check(lib.tok_chan_apply(v, ld, ptr(ds), 0, scale, rpi, images, heads, dk, ld, st), 'tok_chan_apply')   # dk
        _C.check(lib.tok_chan_apply(k, ld, ptr(ds), 1, scale, rpi, images, heads, dv, ld, st), 'tok_chan_apply')   # dv
        if ld != 3 * c:
            tgt[:, 3 * c:] = 0
        self.out.grad = None

    def release(self):
        self.qkv = self.out = self.attn = None


def channel_attention(region: Region, qkv: TTensor, images: int, rows_per_image: int, heads: int) -> TTensor:
    """davit.py:152-165 on qkv rows [B*N][3C]: A = softmax((k * scale)^T v) per (image, head), out = q A^T."""
    c = heads * 32
    if qkv.c != 3 * c:
        raise NotImplementedError('channel_attention: head_dim 32 (every DaViT variant of the reference)')
    lib, st = _C.lib(), stream_ptr()
    dev = qkv.data.device
    ld = qkv.cp
    scale = 32 ** -0.5
    q, k, v = (ptr(qkv.data) + 2 * o for o in (0, c, 2 * c))
    attn = torch.empty((images * heads, 32, 32), dtype=F32, device=dev)
    _C.check(lib.tok_chan_gram(k, ld, v, ld, rows_per_image, images, heads, scale, 1, None, ptr(attn), st), 'tok_chan_gram')
    out_data = torch.empty((images * rows_per_image, c), dtype=BF16, device=dev)
    _C.check(lib.tok_chan_apply(q, ld, ptr(attn), 0, 1.0, rows_per_image, images, heads, ptr(out_data), c, st),
             'tok_chan_apply')
    req = region.grad_mode and qkv.requires_grad
    out = TTensor(out_data, c, requires_grad=req)
    if req:
        node = _ChannelAttnNode()
        node.qkv, node.out, node.attn, node.geo = qkv, out, attn, (images, rows_per_image, heads, c, scale)
        out.node = node
        qkv.uses += 1
        region.add(node)
    return out


class _ResidualNode(Node):
    needs_backward = True

    def backward(self):
        lib, st = _C.lib(), stream_ptr()
        g = self.out.grad
        if g is None:
            return
        a, b = self.a, self.b
        rows, cp = _rows(b), b.cp
        if b.requires_grad:
            tgt, acc = grad_target(b)
            _C.check(lib.tok_scale_rows_add(None, ptr(g), ptr(self.row_scale), self.rps, ptr(tgt), acc, rows, cp, st),
                     'tok_scale_rows_add')
        if a.requires_grad:
            if not (self.out.grad_owned and donate_grad(a, g.view(a.data.shape))):
                tgt, acc = grad_target(a)
                _C.check(lib.tok_act_bwd(2, ptr(g), ptr(g), ptr(tgt), acc, g.numel(), st), 'tok_act_bwd')
        self.out.grad = None

    def release(self):
        self.a = self.b = self.out = self.row_scale = None


def residual_add(region: Region, a: TTensor, b: TTensor, row_scale: Optional[torch.Tensor] = None,
                 rows_per_sample: int = 0) -> TTensor:
    """out = a + row_scale[sample] * b — `x + drop_path(f(x))` with the stochastic-depth keep/scale vector applied in place."""
    lib, st = _C.lib(), stream_ptr()
    rows, cp = _rows(b), b.cp
    if a.data.shape != b.data.shape:
        raise ValueError(f'residual_add: {tuple(a.data.shape)} vs {tuple(b.data.shape)}')
    out_data = torch.empty_like(b.data)
    _C.check(lib.tok_scale_rows_add(ptr(a.data), ptr(b.data), ptr(row_scale), rows_per_sample, ptr(out_data), 0, rows, cp, st),
             'tok_scale_rows_add')
    req = region.grad_mode and (a.requires_grad or b.requires_grad)
    out = TTensor(out_data, b.c, requires_grad=req)
    if req:
        node = _ResidualNode()
        node.a, node.b, node.out, node.row_scale, node.rps = a, b, out, row_scale, rows_per_sample
        out.node = node
        if a.requires_grad:
            a.uses += 1
        if b.requires_grad:
            b.uses += 1
        region.add(node)
    return out


# ---- DaViT ConvPosEnc with activation: depthwise 3x3 + bias ------------------------------------------------------------------
class _DwConvNode(Node):
    needs_backward = True

    def backward(self):
        lib, st = _C.lib(), stream_ptr()
        g = self.out.grad
        if g is None:
            return
        x, conv = self.x, self.conv
        n, h, w, ld = x.shape
        w_need, b_need = conv.weight.requires_grad, conv.bias is not None and conv.bias.requires_grad
        if w_need or b_need:
            blocks = lib.tok_dwconv3x3_wgrad_blocks(n, h)
            partial = torch.empty((blocks, x.c, 10), dtype=F32, device=g.device)
            ws, bs, acc, finish = PG.pair_sinks(conv.weight if w_need else None, conv.bias if b_need else None)
            _C.check(lib.tok_dwconv3x3_wgrad(ptr(x.data), ptr(g), n, h, w, x.c, ld, ptr(partial), ptr(ws), ptr(bs), acc, st),
                     'tok_dwconv3x3_wgrad')
            finish()
        if x.requires_grad:
            tgt, acc = grad_target(x)
            _C.check(lib.tok_dwconv3x3(ptr(g), ptr(conv.weight), None, ptr(tgt), acc, 1, n, h, w, x.c, ld, st), 'tok_dwconv3x3')
        self.out.grad = None

    def release(self):
        self.x = self.out = None


def dwconv3x3(region: Region, x: TTensor, conv: nn.Conv2d) -> TTensor:
    """Depthwise 3x3 / stride 1 / pad 1 convolution (+ bias) on a (B, H, W, C) map."""
    c = x.c
    if (conv.groups != c or conv.in_channels != c or conv.out_channels != c or tuple(conv.kernel_size) != (3, 3) or
            tuple(conv.stride) != (1, 1) or tuple(conv.padding) != (1, 1) or not conv.weight.is_contiguous()):
        raise NotImplementedError('dwconv3x3: depthwise 3x3, stride 1, padding 1')
    n, h, w, ld = x.shape
    y = torch.empty_like(x.data)
    _C.check(_C.lib().tok_dwconv3x3(ptr(x.data), ptr(conv.weight), ptr(conv.bias), ptr(y), 0, 0, n, h, w, c, ld, stream_ptr()),
             'tok_dwconv3x3')
    req = region.grad_mode and (x.requires_grad or conv.weight.requires_grad)
    out = TTensor(y, c, requires_grad=req)
    if req:
        node = _DwConvNode()
        node.x, node.out, node.conv = x, out, conv
        out.node = node
        if x.requires_grad:
            x.uses += 1
        region.add(node)
    return out


# ---- Vision Transformer: global attention, patch embedding, token assembly ---------------------------------------------------
class _GlobalAttnNode(Node):
    needs_backward = True
    bias_node = None        # _RelposBiasNode: the attention ran with its bias; d(bias) is handed to it

    def backward(self):
        lib, st = _C.lib(), stream_ptr()
        g = self.out.grad
        if g is None:
            return
        b, n, heads = self.geo
        qkv, o = self.qkv, self.out
        if g.stride(0) != o.data.stride(0):
            raise RuntimeError('global_attention: d(out) and out do not share a row pitch')
        tgt, acc = grad_target(qkv)
        if acc:
            raise RuntimeError('global_attention: qkv has a single consumer')
        bn = self.bias_node
        what, dbias, bias_args, dbias_args = 'tok_global_attn_bwd', None, (), ()
        if bn is not None:
            bias = bn.gather()             # gathered again: no block keeps its [heads][N][N] bias across the step
            ldb = bias.shape[-1]
            dbias = torch.empty_like(bias) if bn.table.requires_grad else None
            what, bias_args, dbias_args = 'tok_global_attn_bias_bwd', (ptr(bias), ldb), (ptr(dbias), 0)
        # a frozen table needs delta only, not the chunk partials of d(bias)
        ws_bytes = int(lib.tok_global_attn_bwd_ws_bytes(b, n, heads) if dbias is None
                       else lib.tok_global_attn_bias_bwd_ws_bytes(b, n, heads, ldb))
        ws = torch.empty(max(ws_bytes // 4, 1), dtype=F32, device=g.device)
        _C.check(getattr(lib, what)(ptr(qkv.data), qkv.cp, ptr(o.data), ptr(g), o.cp, ptr(self.lse), *bias_args, b, n, heads, 64,
                                    ptr(tgt), qkv.cp, *dbias_args, ptr(ws), ws_bytes, st), what)
        if bn is not None:
            bn.dbias = dbias
        c = heads * 64
        if qkv.cp != 3 * c:
            tgt[:, 3 * c:] = 0
        self.out.grad = None

    def release(self):
        self.qkv = self.out = self.lse = self.bias_node = None


class _RelposBiasNode(Node):
    """The bias of one BEiT attention unit.  `gather()` produces it (forward, and again in the attention unit's backward);
    the attention unit's backward leaves d(bias) here and this unit — recorded before it, so run after it — transposes the
    gather into the table's gradient."""
    needs_backward = True
    dbias = None

    def gather(self) -> torch.Tensor:
        heads, n = self.heads, self.n
        ldb = (n + 3) // 4 * 4
        bias = torch.empty((heads, n, ldb), dtype=F32, device=self.table.device)
        _C.check(_C.lib().tok_relpos_bias_fwd(ptr(self.table.detach()), ptr(self.index), heads, n, ptr(bias), ldb, stream_ptr()),
                 'tok_relpos_bias_fwd')
        return bias

    def backward(self):
        dbias, self.dbias = self.dbias, None
        table = self.table
        if dbias is None or not table.requires_grad:
            return
        slot, acc = PG.sink(table)
        _C.check(_C.lib().tok_relpos_bias_bwd(ptr(dbias), dbias.shape[-1], ptr(self.index), self.heads, self.n, table.shape[0],
                                              ptr(slot), acc, stream_ptr()), 'tok_relpos_bias_bwd')
        PG.commit(table, slot, acc)

    def release(self):
        self.table = self.index = self.dbias = None


def relpos_bias(region: Region, table: nn.Parameter, index: torch.Tensor, heads: int, n_tokens: int, checked: dict = None):
    """[timm 0.6.13] beit.Attention._get_rel_pos_bias: table[index.view(-1)].view(N, N, heads).permute(2, 0, 1) as fp32
    [heads][N][ldb] (ldb = N rounded up to 4; the pad columns are never read).  -> (bias, node); `global_attention` takes the
    pair.  An index outside the table is refused here, on the host (one sync).  `checked` is a dict the caller owns (the attention
    module): the range check is skipped while it records this table height and this very index storage and version."""
    rows = table.shape[0]
    if (tuple(table.shape) != (rows, heads) or not table.is_contiguous() or table.dtype != F32 or index.dtype != torch.int64
            or tuple(index.shape) != (n_tokens, n_tokens) or not index.is_contiguous() or index.device != table.device):
        raise ValueError(f'relpos_bias: table {tuple(table.shape)} / index {tuple(index.shape)} {index.dtype} for {heads} heads, '
                         f'{n_tokens} tokens (fp32 [T][heads], contiguous int64 [N][N] on one device)')
    seen = (rows, index.data_ptr(), index._version, index.device)
    if checked is None or checked.get('relpos_index') != seen:
        lo, hi = int(index.min()), int(index.max())
        if lo < 0 or hi >= rows:
            raise ValueError(f'relpos_bias: relative_position_index holds {lo} ... {hi}, the table has {rows} rows')
        if checked is not None:
            checked['relpos_index'] = seen
    node = _RelposBiasNode()
    node.table, node.index, node.heads, node.n = table, index, heads, n_tokens
    bias = node.gather()
    if not region.grad_mode:
        return bias, None
    region.add(node)
    return bias, node


def global_attention(region: Region, qkv: TTensor, batch: int, tokens: int, heads: int, head_dim: int = 64,
                     bias=None) -> TTensor:
    """[timm 0.6.13] Attention.forward between qkv and proj: qkv rows [B*N][3C] -> softmax(q k^T * 64^-0.5) v rows [B*N][C],
    over all N tokens of an image.  The node keeps qkv, the output and the row log-sum-exp; its backward writes d(qkv).
    bias: the (bias, node) pair of `relpos_bias` — softmax(q k^T * 64^-0.5 + bias[h]) v; the backward gathers the bias again
    and hands d(bias) to that node."""
    c = heads * head_dim
    if qkv.c != 3 * c:
        raise ValueError(f'global_attention: qkv width {qkv.c} != 3 * {heads} heads * {head_dim}')
    lib, st = _C.lib(), stream_ptr()
    dev = qkv.data.device
    out_data = torch.empty((batch * tokens, c), dtype=BF16, device=dev)
    lse = torch.empty((batch, heads, tokens), dtype=F32, device=dev)
    what, bias_args = 'tok_global_attn_fwd', ()
    if bias is not None:
        what = 'tok_global_attn_bias_fwd'
        bias_data = bias[0]
        if tuple(bias_data.shape[:2]) != (heads, tokens):
            raise ValueError(f'global_attention: bias {tuple(bias_data.shape)} for {heads} heads, {tokens} tokens')
        bias_args = (ptr(bias_data), bias_data.shape[-1])
    rc = getattr(lib, what)(ptr(qkv.data), qkv.cp, *bias_args, batch, tokens, heads, head_dim, ptr(out_data), c, ptr(lse), st)
    if rc != 0 and head_dim != 64:
        raise NotImplementedError(f'global_attention: head_dim {head_dim} (64 only)')
    _C.check(rc, what)
    req = region.grad_mode and (qkv.requires_grad or (bias is not None and bias[1] is not None and bias[1].table.requires_grad))
    out = TTensor(out_data, c, requires_grad=req)
    if req:
        node = _GlobalAttnNode()
        node.qkv, node.out, node.lse, node.geo = qkv, out, lse, (batch, tokens, heads)
        if bias is not None:
            node.bias_node = bias[1]
        out.node = node
        qkv.uses += 1
        region.add(node)
    return out


# ---- GCViT: biased window attention with an optional shared query -------------------------------------------------------------
class _GcWindowAttnNode(Node):
    needs_backward = True

    def backward(self):
        lib, st = _C.lib(), stream_ptr()
        g = self.out.grad
        if g is None:
            return
        b, h, w, c, heads, ws = self.geo
        qkv, qg, o, bn = self.qkv, self.q_global, self.out, self.bias_node
        if g.stride(0) != o.data.stride(0):
            raise RuntimeError('gc_window_attention: d(out) and out do not share a row pitch')
        tgt, acc = grad_target(qkv)
        if acc:
            raise RuntimeError('gc_window_attention: qkv has a single consumer')
        bias = bn.gather()                 # gathered again: no block keeps its [heads][N][N] bias across the step
        ldb = bias.shape[-1]
        dbias = torch.empty_like(bias) if bn.table.requires_grad else None
        dqg = qg_tgt = None
        if qg is not None and not qg.requires_grad:
            dqg = torch.empty_like(qg.data)            # the kernel writes it; nobody reads it
        elif qg is not None:
            # q_global has one consumer per global block of its stage: the kernel writes d(q_global) of THIS block, which is the
            # gradient's first contribution or is added to it
            qg_tgt, qg_acc = grad_target(qg)
            dqg = torch.empty_like(qg_tgt) if qg_acc else qg_tgt
        ws_bytes = int(lib.tok_gc_attn_bwd_ws_bytes(b, h, w, heads, ws, int(qg is not None), int(dbias is not None)))
        wsb = torch.empty(max(ws_bytes // 4, 1), dtype=F32, device=g.device)
        _C.check(lib.tok_gc_attn_bwd(ptr(qkv.data), qkv.cp, ptr(qg.data) if qg is not None else None, qg.cp if qg is not None else 0,
                                     ptr(bias), ldb, ptr(o.data), ptr(g), o.cp, ptr(self.lse), b, h, w, c, heads, ws, ptr(tgt),
                                     qkv.cp, ptr(dqg), qg.cp if qg is not None else 0, ptr(dbias), 0, ptr(wsb), ws_bytes, st),
                 'tok_gc_attn_bwd')
        if qg_tgt is not None and dqg is not qg_tgt:
            _C.check(lib.tok_act_bwd(2, ptr(dqg), ptr(dqg), ptr(qg_tgt), 1, dqg.numel(), st), 'tok_act_bwd')
        bn.dbias = dbias
        self.out.grad = None

    def release(self):
        self.qkv = self.q_global = self.out = self.lse = self.bias_node = None


def gc_window_attention(region: Region, qkv: TTensor, geo: Tuple[int, int, int, int, int, int], bias,
                        q_global: Optional[TTensor] = None) -> TTensor:
    """[timm 0.6.13] gcvit.WindowAttentionGlobal.forward between qkv and proj, window_partition / window_reverse included:
    softmax(q k^T * 32^-0.5 + bias[h]) v over the windows of a token map; geo = (B, H, W, C, heads, window).
    q_global None: qkv rows [B*H*W][3C].  q_global given (a (B, ws, ws, C) map): qkv rows [B*H*W][2C] hold k | v and window u
    takes the query of image u mod B — the reference's `repeat`, see csrc/gc_attn.hip.  bias: the (bias, node) pair of
    `relpos_bias`; the backward gathers the bias again and hands d(bias) to that node.  d(q_global) accumulates over its
    consumers (one per global block of a stage)."""
    b, h, w, c, heads, ws = geo
    if c != heads * 32:
        raise NotImplementedError(f'gc_window_attention: head_dim {c // max(heads, 1)} (32 only)')
    if h % ws or w % ws:
        raise NotImplementedError(f'gc_window_attention: a {h}x{w} token map is not a multiple of the window {ws}')
    n = ws * ws
    if n > 256:
        raise NotImplementedError(f'gc_window_attention: {n} tokens per window (at most 256)')
    parts = 3 if q_global is None else 2
    if qkv.c != parts * c or qkv.rows() != b * h * w:
        raise ValueError(f'gc_window_attention: qkv {tuple(qkv.shape)} for {b}x{h}x{w} tokens of {parts} x {c}')
    if q_global is not None and (q_global.c != c or q_global.cp != c or q_global.rows() != b * n):
        raise ValueError(f'gc_window_attention: q_global {tuple(q_global.shape)} for {b} images of {n} x {c}')
    bias_data, bias_node = bias
    if tuple(bias_data.shape[:2]) != (heads, n):
        raise ValueError(f'gc_window_attention: bias {tuple(bias_data.shape)} for {heads} heads, {n} tokens')
    await_ready(qkv, q_global)
    lib, st = _C.lib(), stream_ptr()
    dev = qkv.data.device
    nw = (h // ws) * (w // ws)
    out_data = torch.empty((b * h * w, c), dtype=BF16, device=dev)
    lse = torch.empty((b * nw, heads, n), dtype=F32, device=dev)
    _C.check(lib.tok_gc_attn_fwd(ptr(qkv.data), qkv.cp, ptr(q_global.data) if q_global is not None else None,
                                 q_global.cp if q_global is not None else 0, ptr(bias_data), bias_data.shape[-1], b, h, w, c, heads,
                                 ws, ptr(out_data), c, ptr(lse), st), 'tok_gc_attn_fwd')
    req = region.grad_mode and bias_node is not None and (
        qkv.requires_grad or bias_node.table.requires_grad or (q_global is not None and q_global.requires_grad))
    out = TTensor(out_data, c, requires_grad=bool(req))
    if req:
        node = _GcWindowAttnNode()
        node.qkv, node.q_global, node.out, node.lse, node.geo, node.bias_node = qkv, q_global, out, lse, geo, bias_node
        out.node = node
        qkv.uses += 1
        if q_global is not None and q_global.requires_grad:
            q_global.uses += 1
        region.add(node)
    return out


class _PatchEmbedNode(Node):
    needs_backward = True

    def backward(self):
        lib, st = _C.lib(), stream_ptr()
        g = self.out.grad
        if g is None:
            return
        conv, d, rows = self.conv, self.desc, self.rows
        m, kp = g.shape
        k, p = conv.out_channels, conv.kernel_size[0]
        if conv.bias is not None and conv.bias.requires_grad:
            slot, acc = PG.sink(conv.bias)
            PG.colsum(g, m, kp, slot, acc, two_pass=True)
            PG.commit(conv.bias, slot, acc)
        if conv.weight.requires_grad:
            # the GEMM's weight gradient over the gathered rows is [K][p][p][4]; the master's channels-last slot is [K][p][p][3]
            full = PG.weight_grad(d, rows, g, k, d.c, out=torch.empty((k, p, p, 4), dtype=F32, device=g.device))[0]
            slot, acc = PG.sink(conv.weight)
            PG.store(slot.permute(0, 2, 3, 1), acc, full[..., :conv.in_channels])
            PG.commit(conv.weight, slot, acc)
        self.out.grad = None

    def release(self):
        self.out = self.rows = None


def patch_embed(region: Region, x: TTensor, conv: nn.Conv2d) -> Tuple[TTensor, Tuple[int, int]]:
    """[timm 0.6.13] PatchEmbed.proj (k = p, stride = p, no padding) on the c4 NHWC image: the non-overlapping patches are
    gathered into rows [B*gh*gw][p*p*4] (tok_patch_gather) and multiplied with the [D][p][p][4] weight pack on the 1x1 GEMM.
    -> (token rows [B*gh*gw][D], (gh, gw)).  The image takes no gradient."""
    p = conv.kernel_size[0]
    if (tuple(conv.kernel_size) != (p, p) or tuple(conv.stride) != (p, p) or tuple(conv.padding) != (0, 0) or conv.groups != 1
            or tuple(conv.dilation) != (1, 1) or conv.in_channels > 4 or x.data.dim() != 4 or x.cp != 4):
        raise NotImplementedError('patch_embed: k = stride = p, no padding, at most 3 (4) input channels')
    if x.requires_grad:
        raise NotImplementedError('patch_embed: the image takes no gradient')
    n, h, w, _ = x.shape
    if h % p or w % p:
        raise NotImplementedError(f'patch_embed: a {h}x{w} image is not a multiple of the patch size {p}')
    lib, st = _C.lib(), stream_ptr()
    gh, gw = h // p, w // p
    m, kc = n * gh * gw, p * p * 4
    k = conv.out_channels
    kp = pad8(k)
    if kp != k:
        raise NotImplementedError('patch_embed: embed_dim % 8 == 0')
    rows = torch.empty((m, kc), dtype=BF16, device=x.data.device)
    _C.check(lib.tok_patch_gather(ptr(x.data), n, h, w, p, ptr(rows), st), 'tok_patch_gather')
    pk = get_packs(conv.weight, conv.bias, kp, p, 4, want_dgrad=False, refresh=True)
    d = _C.ConvDesc(m, 1, 1, kc, kp, 1, 1, 1, 1, 1, 0, 1)
    y = torch.empty((m, kp), dtype=BF16, device=x.data.device)
    _C.check(lib.tok_conv_fwd(d, ptr(rows), ptr(pk.fwd), ptr(pk.bias), ptr(y), None, st), 'tok_conv_fwd')
    req = region.grad_mode and (conv.weight.requires_grad or (conv.bias is not None and conv.bias.requires_grad))
    out = TTensor(y, k, requires_grad=req)
    if req:
        node = _PatchEmbedNode()
        node.out, node.conv, node.desc, node.rows = out, conv, d, rows
        out.node = node
        region.add(node)
    return out, (gh, gw)


class _VitEmbedNode(Node):
    needs_backward = True

    def backward(self):
        lib, st = _C.lib(), stream_ptr()
        g = self.out.grad
        if g is None:
            return
        b, n_p, dim, no_embed_class = self.geo
        pos, cls, x = self.pos, self.cls, self.x
        has_cls = cls is not None
        pos_need, cls_need = pos.requires_grad, has_cls and cls.requires_grad
        if pos_need or cls_need:       # a frozen parameter takes no fold at all
            ps, pa = PG.sink(pos) if pos_need else (None, 0)
            cs, ca = PG.sink(cls) if cls_need else (None, 0)
            _C.check(lib.tok_vit_embed_bwd(ptr(g), b, n_p, dim, 1 if has_cls else 0, 1 if no_embed_class else 0, ptr(ps), pa,
                                           ptr(cs), ca, st), 'tok_vit_embed_bwd')
            if pos_need:
                PG.commit(pos, ps, pa)
            if cls_need:
                PG.commit(cls, cs, ca)
        if x.requires_grad:
            tgt, acc = grad_target(x)
            prefix = 1 if has_cls else 0
            if acc:
                tmp = torch.empty_like(tgt)
                _C.check(lib.tok_rows_select(ptr(g), b, n_p + prefix, prefix, n_p, dim, ptr(tmp), 0, 0, st), 'tok_rows_select')
                _C.check(lib.tok_act_bwd(2, ptr(tmp), ptr(tmp), ptr(tgt), 1, tmp.numel(), st), 'tok_act_bwd')
            else:
                _C.check(lib.tok_rows_select(ptr(g), b, n_p + prefix, prefix, n_p, dim, ptr(tgt), 0, 0, st), 'tok_rows_select')
        self.out.grad = None

    def release(self):
        self.x = self.out = self.pos = self.cls = None


def vit_embed(region: Region, x: TTensor, batch: int, pos_embed: nn.Parameter, cls_token: Optional[nn.Parameter],
              no_embed_class: bool = False) -> TTensor:
    """VisionTransformer._pos_embed (vit.py:284-298) on patch rows [B*P][D]: prepend the class token and add the position
    embedding, rounded once -> token rows [B*T][D] (T = P + 1 with a class token).  Frozen parameters take no fold."""
    dim = x.c
    if x.cp != dim or dim % 8:
        raise NotImplementedError('vit_embed: embed_dim % 8 == 0')
    n_p = x.rows() // batch
    prefix = 1 if cls_token is not None else 0
    want = n_p if no_embed_class else n_p + prefix
    if pos_embed.numel() != want * dim or not pos_embed.is_contiguous():
        raise ValueError(f'vit_embed: pos_embed {tuple(pos_embed.shape)} does not hold {want} x {dim} (contiguous)')
    if cls_token is not None and (cls_token.numel() != dim or not cls_token.is_contiguous()):
        raise ValueError(f'vit_embed: cls_token {tuple(cls_token.shape)}')
    out_data = torch.empty((batch * (n_p + prefix), dim), dtype=BF16, device=x.data.device)
    _C.check(_C.lib().tok_vit_embed_fwd(ptr(x.data), ptr(pos_embed.detach()), ptr(cls_token.detach()) if prefix else None, batch,
                                        n_p, dim, 1 if no_embed_class else 0, ptr(out_data), stream_ptr()), 'tok_vit_embed_fwd')
    req = region.grad_mode and (x.requires_grad or pos_embed.requires_grad or (prefix and cls_token.requires_grad))
    out = TTensor(out_data, dim, requires_grad=bool(req))
    if req:
        node = _VitEmbedNode()
        node.x, node.out, node.pos, node.cls, node.geo = x, out, pos_embed, cls_token, (batch, n_p, dim, no_embed_class)
        out.node = node
        if x.requires_grad:
            x.uses += 1
        region.add(node)
    return out


class _RowsSelectNode(Node):
    needs_backward = True

    def backward(self):
        g = self.out.grad
        if g is None or not self.x.requires_grad:
            return
        b, t, first, count = self.geo
        tgt, acc = grad_target(self.x)
        _C.check(_C.lib().tok_rows_select(ptr(g), b, t, first, count, self.x.cp, ptr(tgt), 1, acc, stream_ptr()),
                 'tok_rows_select')
        self.out.grad = None

    def release(self):
        self.x = self.out = None


def rows_select(region: Region, x: TTensor, batch: int, first: int, count: int) -> TTensor:
    """Rows [first, first + count) of every image's token rows: x[:, first:first + count] of the (B, T, C) view (the class
    token the final norm reads, or the patch tokens of forward_features)."""
    t = x.rows() // batch
    y = torch.empty((batch * count, x.cp), dtype=BF16, device=x.data.device)
    _C.check(_C.lib().tok_rows_select(ptr(x.data), batch, t, first, count, x.cp, ptr(y), 0, 0, stream_ptr()), 'tok_rows_select')
    req = region.grad_mode and x.requires_grad
    out = TTensor(y, x.c, requires_grad=req)
    if req:
        node = _RowsSelectNode()
        node.x, node.out, node.geo = x, out, (batch, t, first, count)
        out.node = node
        x.uses += 1
        region.add(node)
    return out


# ---- BEiT: LayerScale residual ------------------------------------------------------------------------------------------------
class _LayerScaleNode(Node):
    needs_backward = True

    def backward(self):
        lib, st = _C.lib(), stream_ptr()
        g = self.out.grad
        if g is None:
            return
        x, a, gamma = self.x, self.a, self.gamma
        rows, d = _rows(a), a.cp
        g_need = gamma.requires_grad
        if a.requires_grad or g_need:
            tgt, acc = grad_target(a) if a.requires_grad else (None, 0)
            slot, gacc = PG.sink(gamma) if g_need else (None, 0)
            part = torch.empty((lib.tok_layer_scale_bwd_rows(rows, d), d), dtype=F32, device=g.device) if g_need else None
            _C.check(lib.tok_layer_scale_bwd(ptr(g), ptr(a.data), ptr(gamma.detach()), ptr(self.row_scale), self.rps, ptr(tgt), acc,
                                             ptr(slot), gacc, ptr(part), rows, d, st), 'tok_layer_scale_bwd')
            if g_need:
                PG.commit(gamma, slot, gacc)
        if x.requires_grad:
            if not (self.out.grad_owned and donate_grad(x, g.view(x.data.shape))):
                tgt, acc = grad_target(x)
                _C.check(lib.tok_act_bwd(2, ptr(g), ptr(g), ptr(tgt), acc, g.numel(), st), 'tok_act_bwd')
        self.out.grad = None

    def release(self):
        self.x = self.a = self.out = self.row_scale = self.gamma = None


def layer_scale_add(region: Region, x: TTensor, a: TTensor, gamma: nn.Parameter, row_scale: Optional[torch.Tensor] = None,
                    tokens: int = 0) -> TTensor:
    """out = x + row_scale[sample] * gamma * a — [timm 0.6.13] beit.Block's  x + drop_path(gamma_i * f(norm(x)))  with the
    stochastic-depth keep/scale vector applied in place (`tokens` rows per sample).  gamma: the fp32 [dim] parameter."""
    lib, st = _C.lib(), stream_ptr()
    rows, d = _rows(a), a.cp
    if x.data.shape != a.data.shape:
        raise ValueError(f'layer_scale_add: {tuple(x.data.shape)} vs {tuple(a.data.shape)}')
    if gamma.numel() != d or gamma.dtype != F32 or not gamma.is_contiguous():
        raise ValueError(f'layer_scale_add: gamma {tuple(gamma.shape)} {gamma.dtype} for rows of {d} (fp32, contiguous)')
    out_data = torch.empty_like(a.data)
    _C.check(lib.tok_layer_scale_fwd(ptr(x.data), ptr(a.data), ptr(gamma.detach()), ptr(row_scale), tokens, ptr(out_data), rows, d,
                                     st), 'tok_layer_scale_fwd')
    req = region.grad_mode and (x.requires_grad or a.requires_grad or gamma.requires_grad)
    out = TTensor(out_data, a.c, requires_grad=req)
    if req:
        node = _LayerScaleNode()
        node.x, node.a, node.out, node.gamma, node.row_scale, node.rps = x, a, out, gamma, row_scale, tokens
        out.node = node
        if x.requires_grad:
            x.uses += 1
        if a.requires_grad:
            a.uses += 1
        region.add(node)
    return out
