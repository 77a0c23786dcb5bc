"""The grouped 3x3 convolution of csrc/conv_group.hip stated in fp64, and the launch geometry its error bounds need.

The three operations are torch's own grouped convolution and its two gradients on the values the kernels multiply: x, dout
and the weight rounded to bf16, cast to double.  Nothing here runs on the GPU or reads the library."""
import torch
import torch.nn.functional as F

BF = torch.bfloat16
WIDTHS = (4, 8, 16, 32, 64)            # group widths the kernels serve


def odim(h, stride):
    return (h - 1) // stride + 1


def nhwc(t):
    """(N, C, H, W) -> [N H W][C], the kernels' row order"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


class Ref:
    """fp64 results and magnitude terms (the same sums over absolute values) of one layer.
    x (n, h, w, c) bf16, w (c, cg, 3, 3) fp32 (rounded to bf16 here, as the kernels do), dout (n, p, q, c) bf16."""

    def __init__(self, x, w, dout, groups, stride):
        c = x.shape[-1]
        xd, gd = x.double().permute(0, 3, 1, 2), dout.double().permute(0, 3, 1, 2)
        wd = w.to(BF).double()
        kw = dict(stride=stride, padding=1, groups=groups)
        self.out = nhwc(F.conv2d(xd, wd, **kw))
        self.out_mag = nhwc(F.conv2d(xd.abs(), wd.abs(), **kw))
        self.dx = nhwc(torch.nn.grad.conv2d_input(xd.shape, wd, gd, **kw))
        self.dx_mag = nhwc(torch.nn.grad.conv2d_input(xd.shape, wd.abs(), gd.abs(), **kw))
        self.dw = torch.nn.grad.conv2d_weight(xd, wd.shape, gd, **kw)                    # (c, cg, 3, 3)
        self.dw_mag = torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, gd.abs(), **kw)
        assert self.out.shape[1] == c


def stats_ref(out_rounded):
    """column sums of the statistics rows: sum and sum of squares of the ROUNDED output [m][c], and their magnitudes"""
    o = out_rounded.double()
    return o.sum(0), (o * o).sum(0), o.abs().sum(0)


# ---- the launch geometry of csrc/conv_group.hip, restated ------------------------------------------------------------------
FWD_BLOCKS, WG_WAVES = 1024, 2048
PIX_TILE, WG_CHUNK = 16, 32            # pixels of a forward / data-gradient tile, of a weight-gradient chunk (one MFMA's K)


def cdiv(a, b):
    return -(-a // b)


def geo(pixels, c, groups):
    """forward / data gradient over `pixels` result pixels: grid (gx, rows), 16-pixel tiles, tiles a wave walks at most"""
    cg = c // groups
    ic = max(cg, 16)
    ctiles = cdiv(c, 16)
    gx = cdiv(ctiles, 4)
    ptiles = cdiv(pixels, PIX_TILE)
    rows = min(ptiles, max(FWD_BLOCKS // gx, 1))
    return dict(cg=cg, ic=ic, ctiles=ctiles, gx=gx, ptiles=ptiles, rows=rows, trips=cdiv(ptiles, rows))


def wgrad_geo(pixels, c, groups):
    """weight gradient over `pixels` forward-output pixels: (output tile, input tile) pairs, 32-pixel chunks, workspace rows"""
    g = geo(pixels, c, groups)
    npairs = g['ctiles'] * (g['ic'] // 16)
    chunks = cdiv(pixels, WG_CHUNK)
    rows = min(chunks, max(WG_WAVES // npairs, 1))
    return dict(npairs=npairs, chunks=chunks, rows=rows, trips=cdiv(chunks, rows), ws_bytes=rows * npairs * 9 * 256 * 4)


def stats_chain(g):
    """longest chain of dependent fp32 additions inside one statistics row: the tiles a lane walks, then the 16 pixel lanes
    folded in order (the rows themselves are folded by the test in fp64; tok_bn_finalize has its own contract)"""
    return g['trips'] + PIX_TILE


def wgrad_chain(wg):
    """... of a weight-gradient element: the 32 products of each chunk an accumulator takes, then the workspace rows in order"""
    return wg['trips'] * WG_CHUNK + wg['rows']
