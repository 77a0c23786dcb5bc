"""Kernel contract of tok_phase_split / tok_phase_merge (csrc/phase.hip), element by element.  Without `accumulate` both are
copies: random 16-bit patterns (NaN payloads, infinities, -0 among them) compared as int16 against torch indexing.  With it the
destination becomes bf16(float(old) + float(v)), rounded once: bit for bit on finite data.  Operands sit in helpers.Mat buffers:
input pads and guards hold NaN (which must never appear), output pads and guards hold sentinels that are checked after the call.
Also: merge(split(x)) == x and the converse, reruns bit-identical, a shape past the grid cap of the grid-strided kernel, one
past 2^31 elements, and every refusal writing nothing."""
import pytest
import torch

from helpers import BF, ERR_INVALID, SENTINEL, Mat, last_error
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
I16 = torch.int16
# (n, h, w, c, ld, d): one pixel per phase; pad channels; d = 4 over three images; pad channels at d = 4 with 5 channel groups;
# 2048 channels (256 lanes per pixel)
SHAPES = [(1, 2, 2, 8, 8, 2), (2, 4, 6, 8, 16, 2), (3, 8, 4, 24, 24, 4), (1, 12, 20, 40, 48, 4), (1, 4, 4, 2048, 2048, 2)]
_ids = lambda s: 'x'.join(map(str, s))      # noqa: E731


def split_ref(x, d):
    """[n][h][w][c] -> [n*d*d][h/d][w/d][c] by torch indexing: image (i, a, b) = x[i, a::d, b::d]"""
    n, h, w, c = x.shape
    return torch.stack([x[i, a::d, b::d] for i in range(n) for a in range(d) for b in range(d)])


def merge_ref(xs, n, d):
    _, hq, wq, c = xs.shape
    out = xs.new_empty((n, hq * d, wq * d, c))
    for i in range(n):
        for a in range(d):
            for b in range(d):
                out[i, a::d, b::d] = xs[(i * d + a) * d + b]
    return out


def _patterns(shape, seed):
    """random 16-bit patterns as int16 (the sentinel's own pattern left out: Mat.done takes it for 'never written')"""
    bits = torch.randint(-32768, 32768, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int32).to(I16)
    bits[bits == SENTINEL[BF]] += 1
    return bits


def _mat(rows, c, ld, bits=None, nan=False):
    m = Mat(rows, c, ld, nan=nan)
    if bits is not None:
        m.view.view(I16).copy_(bits.reshape(rows, c).cuda())
    return m


def _call(fn, name, src, shape, dst, accumulate=0):
    n, h, w, c, ld, d = shape
    _C.check(fn(src.ptr, n, h, w, c, ld, d, dst.ptr, accumulate, stream_ptr()), name)
    torch.cuda.synchronize()


def _bits(m, shape4):
    return m.value().view(I16).reshape(shape4)


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_split_and_merge_are_copies_bit_for_bit(shape):
    n, h, w, c, ld, d = shape
    lib = _C.lib()
    rows = n * h * w
    plain, phased = (n, h, w, c), (n * d * d, h // d, w // d, c)
    x = _patterns(plain, 11 + h * w + c)
    assert bool((x.view(BF).float().isnan()).any()) or x.numel() < 512      # NaN payloads are among the patterns
    src = _mat(rows, c, ld, x, nan=True)
    # split: against torch indexing, pads / guards untouched, a rerun gives the same bits
    out = _mat(rows, c, ld)
    _call(lib.tok_phase_split, 'tok_phase_split', src, shape, out)
    out.done('split', finite=False)
    want = split_ref(x, d)
    assert torch.equal(_bits(out, phased), want)
    again = _mat(rows, c, ld)
    _call(lib.tok_phase_split, 'tok_phase_split', src, shape, again)
    assert torch.equal(_bits(again, phased), want)
    # merge(split(x)) == x
    back = _mat(rows, c, ld)
    _call(lib.tok_phase_merge, 'tok_phase_merge', out, shape, back)
    back.done('merge(split)', finite=False)
    assert torch.equal(_bits(back, plain), x)
    # merge: a phased tensor of its own, against torch indexing; split(merge(y)) == y
    y = _patterns(phased, 13 + h * w + c)
    ysrc = _mat(rows, c, ld, y, nan=True)
    m = _mat(rows, c, ld)
    _call(lib.tok_phase_merge, 'tok_phase_merge', ysrc, shape, m)
    m.done('merge', finite=False)
    assert torch.equal(_bits(m, plain), merge_ref(y, n, d))
    conv = _mat(rows, c, ld)
    _call(lib.tok_phase_split, 'tok_phase_split', m, shape, conv)
    conv.done('split(merge)', finite=False)
    assert torch.equal(_bits(conv, phased), y)


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_accumulate_is_the_fp32_add_rounded_once(shape):
    n, h, w, c, ld, d = shape
    lib = _C.lib()
    rows = n * h * w
    plain, phased = (n, h, w, c), (n * d * d, h // d, w // d, c)
    g = torch.Generator().manual_seed(17 + h * w + c)
    v = (torch.randn(plain, generator=g) * 3).to(BF)
    old = (torch.randn(phased, generator=g) * 3).to(BF)
    src = Mat(rows, c, ld, init=v.cuda(), nan=True)
    dst = Mat(rows, c, ld, init=old.cuda())
    _call(lib.tok_phase_split, 'tok_phase_split', src, shape, dst, accumulate=1)
    dst.done('split +=')
    want = (old.float() + split_ref(v, d).float()).to(BF)
    assert torch.equal(_bits(dst, phased), want.view(I16))
    # the other direction, on the same data: old (phased) is the source, v (plain) what is accumulated into
    src2 = Mat(rows, c, ld, init=old.cuda(), nan=True)
    dst2 = Mat(rows, c, ld, init=v.cuda())
    _call(lib.tok_phase_merge, 'tok_phase_merge', src2, shape, dst2, accumulate=1)
    dst2.done('merge +=')
    want2 = (v.float() + merge_ref(old, n, d).float()).to(BF)
    assert torch.equal(_bits(dst2, plain), want2.view(I16))


def test_a_shape_past_the_grid_cap():
    """16 908 288 lanes of work against the 65 536 x 256 = 16 777 216 threads of the capped grid: the tail is the grid stride's"""
    n, h, w, c, d = 2, 1024, 1032, 64, 4
    assert n * h * w * (c // 8) > 65536 * 256
    lib, st = _C.lib(), stream_ptr()
    x = torch.randint(-32768, 32768, (n, h, w, c), dtype=torch.int32, device='cuda').to(I16)
    out = torch.zeros((n * d * d, h // d, w // d, c), dtype=I16, device='cuda')
    _C.check(lib.tok_phase_split(x.data_ptr(), n, h, w, c, c, d, out.data_ptr(), 0, st), 'tok_phase_split')
    for i in range(n):
        for a in range(d):
            for b in range(d):
                assert torch.equal(out[(i * d + a) * d + b], x[i, a::d, b::d]), (i, a, b)
    back = torch.zeros_like(x)
    _C.check(lib.tok_phase_merge(out.data_ptr(), n, h, w, c, c, d, back.data_ptr(), 0, st), 'tok_phase_merge')
    torch.cuda.synchronize()
    assert torch.equal(back, x)


def test_offsets_past_2_31_elements():
    """[1][2048][2048][520]: 2.18e9 elements, the shape tests/test_nearest_contract_gpu.py uses: the last rows of either layout
    start past 2^31, where a 32-bit element offset goes wrong.  Eight channels of the 520 move; every phase image and the merge
    back are checked everywhere."""
    n, h, w, c, ld, d = 1, 2048, 2048, 8, 520, 2
    assert n * h * w * ld > 2 ** 31
    lib, st = _C.lib(), stream_ptr()
    x = torch.empty((n, h, w, ld), dtype=I16, device='cuda')
    x[..., :c] = torch.randint(-32768, 32768, (n, h, w, c), dtype=torch.int32, device='cuda').to(I16)
    out = torch.empty((n * d * d, h // d, w // d, ld), dtype=I16, device='cuda')
    out[..., :c] = 0
    _C.check(lib.tok_phase_split(x.data_ptr(), n, h, w, c, ld, d, out.data_ptr(), 0, st), 'tok_phase_split')
    for a in range(d):
        for b in range(d):
            assert torch.equal(out[a * d + b, :, :, :c], x[0, a::d, b::d, :c]), (a, b)
    back = torch.empty_like(x)
    back[..., :c] = 0
    _C.check(lib.tok_phase_merge(out.data_ptr(), n, h, w, c, ld, d, back.data_ptr(), 0, st), 'tok_phase_merge')
    torch.cuda.synchronize()
    assert torch.equal(back[..., :c], x[..., :c])


_OK = dict(n=2, h=4, w=8, c=8, ld=16, d=2)
_BAD = [dict(d=1), dict(d=3), dict(d=8), dict(d=4, h=6), dict(w=7), dict(h=0), dict(c=0), dict(c=4), dict(c=12), dict(c=24),
        dict(ld=12), dict(n=0), dict(n=-1), dict(n=1 << 19, h=64, w=64), dict(x=None), dict(out=None), dict(x='odd'),
        dict(out='odd'), dict(out='x')]


@pytest.mark.parametrize('bad', _BAD, ids=lambda d: ','.join(f'{k}={v}' for k, v in d.items()))
def test_refusals(bad):
    """d outside {2, 4}, a map d does not divide, c or ld no multiple of 8, c > ld, n < 1, 2^31 pixels, a null, misaligned or
    aliased pointer: the invalid-argument code, the entry's name in tok_last_error, and nothing written"""
    lib, st = _C.lib(), stream_ptr()
    a = dict(_OK, **{k: v for k, v in bad.items() if k not in ('x', 'out')})
    x, out = Mat(2 * 4 * 8, 16, 16), Mat(2 * 4 * 8, 16, 16)              # both hold sentinels: a write to either shows
    ptrs = {None: None, 'odd': None, 'x': x.ptr}
    xp = x.ptr + 2 if bad.get('x') == 'odd' else (None if 'x' in bad else x.ptr)
    op = out.ptr + 2 if bad.get('out') == 'odd' else (ptrs[bad['out']] if 'out' in bad else out.ptr)
    for fn, name in ((lib.tok_phase_split, 'tok_phase_split'), (lib.tok_phase_merge, 'tok_phase_merge')):
        for accumulate in (0, 1):
            rc = fn(xp, a['n'], a['h'], a['w'], a['c'], a['ld'], a['d'], op, accumulate, st)
            assert rc == ERR_INVALID and name in last_error(), (name, rc, last_error())
    torch.cuda.synchronize()
    x.intact('refused call')
    out.intact('refused call')
