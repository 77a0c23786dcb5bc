"""The window-attention kernels (csrc/window_attn.hip: two MFMA kernels for windows of up to 64 tokens, two scalar ones above)
across the contract of include/tok.h, element by element against the fp64 reference of tests/window_attn_ref.py (whose
docstring derives every bound; tests/test_window_attn_ref.py shows that an exact kernel with the device's operand formats
stays inside half of each).  Covered here and nowhere else: non-square maps, workgroups that walk 2 / 3 / 16 images with a
shorter last group, N = 81 on the scalar path (its loops stride 64), pitches above 3c with NaN pads, guard rows behind every
output, the d(logits) scratch rows and the d(logit_scale) partials, sharp and masked logits, a zero output gradient and the
argument refusals.  The device backward gets the device forward's log-sum-exp, as in training.
Found while writing it: the refusals of tok_window_attn_fwd / _bwd reported one catch-all message; they now name the argument."""
import pytest
import torch

from helpers import BF, F32, SENTINEL, Guarded, _INT_OF, assert_bounded, cdiv, last_error
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr
from window_attn_ref import HD, WinRef, check_result, make_inputs

pytestmark = pytest.mark.gpu
P = lambda t: None if t is None else t.data_ptr()       # noqa: E731


def _all_written(g, what):
    left = int((g.buf.view(_INT_OF[g.dtype])[:g.rows, :g.cols] == SENTINEL[g.dtype]).sum())
    assert left == 0, f'{what}: {left} owned elements never written'
    assert torch.isfinite(g.view.float()).all(), f'{what}: not finite'


def _launch(dims, qkv, dout, ls, bias, mask, backward=True):
    """forward + backward on guarded buffers: qkv at pitch 3c + 8 (forward) / 3c + 16 (backward, the pitch of dqkv) with NaN
    pads, NaN guard rows behind qkv and dout, sentinels in every output, its pads and its guard row"""
    b, h, w, heads, ws, shift = dims
    lib, st = _C.lib(), stream_ptr()
    c, n, nw, rows = heads * HD, ws * ws, (h // ws) * (w // ws), b * h * w
    ldq, ldd = 3 * c + 8, 3 * c + 16
    dev = [None if t is None else t.cuda() for t in (ls, bias, mask)]
    qg = Guarded(rows, 3 * c, ldq, init=qkv.cuda(), nan_pad=True)
    og = Guarded(rows, c)
    lg = Guarded(b * nw * heads, n, dtype=F32)
    _C.check(lib.tok_window_attn_fwd(qg.ptr, b, h, w, c, heads, ws, shift, ldq, P(dev[0]), P(dev[1]), P(dev[2]), og.ptr, lg.ptr,
                                     st), 'fwd')
    torch.cuda.synchronize()
    for g, what in ((qg, 'qkv'), (og, 'out'), (lg, 'lse')):
        g.check(what)
    _all_written(og, 'out')
    _all_written(lg, 'lse')
    if not backward:
        return og.value(), lg.value(), None, None, None
    r = lib.tok_window_attn_bwd_rows(b, h, w, heads, ws)
    assert 0 < r <= b * nw
    q2 = Guarded(rows, 3 * c, ldd, init=qkv.cuda(), nan_pad=True)
    gg = Guarded(rows, c, init=dout.cuda(), nan_pad=True)
    dg = Guarded(rows, 3 * c, ldd)
    plain = ls is None
    sg = None if plain else Guarded(r, heads * n * n, dtype=F32)
    pg = None if plain else Guarded(r, heads, dtype=F32)
    _C.check(lib.tok_window_attn_bwd(q2.ptr, gg.ptr, b, h, w, c, heads, ws, shift, ldd, P(dev[0]), P(dev[1]), P(dev[2]), lg.ptr,
                                     dg.ptr, None if plain else sg.ptr, None if plain else pg.ptr, st), 'bwd')
    torch.cuda.synchronize()
    for g, what in ((q2, 'qkv'), (gg, 'dout'), (lg, 'lse'), (dg, 'dqkv')) + (() if plain else ((sg, 'ds_scratch'), (pg, 'dscale_part'))):
        g.check(what)
        if g not in (q2, gg):
            _all_written(g, what)
    return og.value(), lg.value(), dg.value(), sg, pg


def _expect_rows(dims, bpw):
    """the case must run the path it names: tok_window_attn_bwd_rows == ceil(B / bpw) * nW at the divisor 1536 / cap 16"""
    b, h, w, heads, ws, _ = dims
    nw = (h // ws) * (w // ws)
    assert bpw == max(1, min(16, b * nw * heads // 1536, b))
    got = _C.lib().tok_window_attn_bwd_rows(b, h, w, heads, ws)
    assert got == cdiv(b, bpw) * nw, (f'{got} scratch rows, {cdiv(b, bpw) * nw} expected for {bpw} images per workgroup: has '
                                      f'attn_bpw (csrc/window_attn.hip) left divisor 1536 / cap 16?')
    return got


def _case(tag, dims, seed, bpw=None, colsum=False, **kw):
    heads, n = dims[3], dims[4] ** 2
    qkv, dout, ls, bias, mask = make_inputs(*dims, seed=seed, **kw)
    if bpw is not None:
        _expect_rows(dims, bpw)
    out, lse, dqkv, sg, pg = _launch(dims, qkv, dout, ls, bias, mask)
    ref = WinRef(qkv, dout, *dims, ls, bias, mask, bpw=bpw or 1)
    dbias = dls = scr = part = None
    if ls is not None:
        scr, part = sg.value(), pg.value()                                # every scratch row is checked on its own ...
        dbias = scr.double().sum(0).view(heads, n, n)                     # ... and the fp64 host fold of the R rows
        dls = part.double().sum(0)
    res = check_result(f'winattn_contract/{tag}', ref, out, lse, dqkv, dbias, dls, scr, part)
    if colsum:                                                            # ... and the fold the engine does
        lib, st = _C.lib(), stream_ptr()
        red = Guarded(1, heads * n * n, dtype=F32)
        _C.check(lib.tok_colsum_f32(sg.ptr, sg.rows, heads * n * n, red.ptr, 0, st), 'colsum')
        torch.cuda.synchronize()
        red.check('d(bias) fold')
        folded = red.value().double().view(heads, n, n)
        assert (folded - dbias).abs().max() <= 2.0 ** -23 * dbias.abs().max()        # one fp32 rounding of the fp64 sum
        check_result(f'winattn_contract/{tag}_colsum', ref, out, lse, dqkv, folded, dls)
    return res


# ---- non-square maps, one image per workgroup (3 / 6 / 12 units: some of the 8 * ceil(units / 8) workgroups are surplus) ----
@pytest.mark.parametrize('b,h,w,heads,ws,shift', [(2, 8, 12, 3, 4, 0), (2, 8, 12, 3, 4, 2), (1, 14, 21, 2, 7, 3),
                                                  (1, 16, 8, 1, 8, 4)])
def test_non_square_maps(b, h, w, heads, ws, shift):
    _case(f'b{b}_{h}x{w}_ws{ws}_h{heads}_s{shift}', (b, h, w, heads, ws, shift), seed=h + w + shift, bpw=1, colsum=(shift == 2))


# ---- several images per workgroup: the prefetch of image b + 1, the d(logits) sum over the images, the shorter last group ----
@pytest.mark.parametrize('b,h,w,heads,ws,shift,plain,bpw', [
    (257, 8, 8, 3, 4, 2, 0, 2),          # N = 16: 3084 units, 128 groups of two images and one of one
    (257, 14, 14, 3, 7, 3, 0, 2),        # N = 49
    (257, 14, 14, 3, 7, 0, 1, 2),        # the same in plain mode
    (386, 8, 8, 12, 8, 0, 0, 3),         # N = 64, nW = 1: 4632 units (12 heads: 3 x 1536 needs them at this batch); last group two
    (1031, 8, 8, 6, 4, 0, 0, 16),        # 24744 units: the cap of 16, last group seven
])
def test_images_per_workgroup(b, h, w, heads, ws, shift, plain, bpw):
    _case(f'b{b}_{h}x{w}_ws{ws}_h{heads}_s{shift}' + ('_plain' if plain else ''), (b, h, w, heads, ws, shift), seed=b,
          bpw=bpw, plain=bool(plain))


# ---- the scalar kernels (N > 64): N = 81 is no multiple of their stride of 64; head 0 sits above the ln 100 clamp ----
@pytest.mark.parametrize('b,h,w,heads,ws,shift', [(2, 9, 18, 2, 9, 4), (1, 16, 32, 1, 16, 8)])
def test_scalar_path(b, h, w, heads, ws, shift):
    dims = (b, h, w, heads, ws, shift)
    assert _C.lib().tok_window_attn_bwd_rows(b, h, w, heads, ws) == b * (h // ws) * (w // ws)
    _case(f'scalar_b{b}_{h}x{w}_ws{ws}', dims, seed=ws, ls0=5.0)


@pytest.mark.parametrize('ws', [4, 7, 8])
def test_forward_at_the_clamped_scale(ws):
    """scale 100 on the MFMA path (head 0): out and lse keep their bounds, which carry Delta"""
    dims = (2, ws, 2 * ws, 2, ws, 0)
    qkv, dout, ls, bias, mask = make_inputs(*dims, seed=ws, ls0=5.0)
    out, lse, *_ = _launch(dims, qkv, dout, ls, bias, mask, backward=False)
    ref = WinRef(qkv, dout, *dims, ls, bias, mask)
    tag = f'winattn_contract/clamped_fwd_ws{ws}'
    assert_bounded(out, ref.out, ref.m_out, 2.0 ** -8, 1.0, 'out', tag)
    assert_bounded(lse.double().view(ref.lse.shape), ref.lse, ref.delta + 2.0 ** -18 * (1 + ref.lse.abs()), 0.0, 1.0, 'lse', tag)


@pytest.mark.parametrize('dims', [(3, 8, 12, 3, 4, 2), (1, 9, 18, 2, 9, 4)], ids=['mfma', 'scalar'])
def test_zero_output_gradient(dims):
    qkv, dout, ls, bias, mask = make_inputs(*dims, seed=3)
    _, _, dqkv, sg, pg = _launch(dims, qkv, torch.zeros_like(dout), ls, bias, mask)
    assert (dqkv == 0).all() and (sg.value() == 0).all() and (pg.value() == 0).all()


@pytest.mark.parametrize('dims,head', [((2, 8, 12, 3, 4, 2), 1), ((1, 14, 21, 2, 7, 3), 0)], ids=['n16', 'n49'])
def test_sharp_logits(dims, head):
    """one head's bias puts +60 on a single key per query (rows nearly one-hot); the -100 shift mask removes whole key ranges"""
    res = _case(f'sharp_{dims[1]}x{dims[2]}_ws{dims[4]}', dims, seed=17, sharp_head=head)
    qkv, dout, ls, bias, mask = make_inputs(*dims, seed=17, sharp_head=head)
    assert (mask == -100).any() and (bias[head].amax(-1) > 50).all()
    assert res['out'] <= 1


def _refused(rc, reason):
    err = last_error()
    assert rc == -1, (rc, err)
    assert reason in err, (reason, err)


def test_refusals():
    """TOK_ERR_INVALID, tok_last_error() names the reason, nothing is written"""
    lib, st = _C.lib(), stream_ptr()
    b, h, w, heads, ws = 1, 8, 8, 2, 4
    c, n, nw = heads * HD, ws * ws, 4
    big = 3 * c + 64
    qkv = torch.zeros(b * 16 * 16, big, dtype=BF, device='cuda')         # large enough for every geometry tried below
    ls, bias = torch.zeros(heads, device='cuda'), torch.zeros(heads, 256, 256, device='cuda')
    mask = torch.zeros(nw, 256, 256, device='cuda')
    outs = [Guarded(b * 16 * 16, big), Guarded(4096, 256, dtype=F32), Guarded(b * 16 * 16, big), Guarded(16, heads * 256 * 4, dtype=F32),
            Guarded(64, heads, dtype=F32)]
    og, lg, dg, sg, pg = outs

    def fwd(h=h, w=w, c=c, heads=heads, ws=ws, shift=0, ld=3 * c, ls=ls, bias=bias, mask=None):
        return lib.tok_window_attn_fwd(P(qkv), b, h, w, c, heads, ws, shift, ld, P(ls), P(bias), P(mask), og.ptr, lg.ptr, st)

    def bwd(h=h, w=w, c=c, heads=heads, ws=ws, shift=0, ld=3 * c, ls=ls, bias=bias, mask=None, scratch=True):
        return lib.tok_window_attn_bwd(P(qkv), P(qkv), b, h, w, c, heads, ws, shift, ld, P(ls), P(bias), P(mask), lg.ptr, dg.ptr,
                                       sg.ptr if scratch else None, pg.ptr if scratch else None, st)
    for f in (fwd, bwd):
        _refused(f(c=c + 32), 'heads * 32')
        _refused(f(h=10), 'multiples of the window')
        _refused(f(w=10), 'multiples of the window')
        _refused(f(shift=ws), 'shift')
        _refused(f(ld=3 * c - 8), 'at least 3c')
        _refused(f(ld=3 * c + 4), 'multiple of 8')
        _refused(f(bias=None), 'go together')                                   # logit_scale without bias
        _refused(f(ls=None, bias=None, mask=mask), 'plain mode')
        _refused(f(ls=None, bias=None, shift=2), 'plain mode')
        _refused(f(ls=None, bias=None, h=9, w=9, ws=9), 'plain mode')           # N = 81
    _refused(fwd(ls=None), 'go together')                                       # bias without logit_scale
    _refused(bwd(scratch=False), 'ds_scratch')
    torch.cuda.synchronize()
    for g in outs:
        assert bool((g.buf.view(_INT_OF[g.dtype]) == SENTINEL[g.dtype]).all()), 'a refused call wrote to an output'
