"""Kernel contract of csrc/layout.hip.  Everything here is exact: every reference is built with torch indexing and
`.to(torch.bfloat16)` (round to nearest even, overflow to inf, NaN kept), never with the host stand-in of the library, and every
comparison is bit for bit.  Sources sit between NaN guards, destinations are filled with sentinels between sentinel guards, so a
pad that is left unwritten, a value taken from outside the operand and a store outside it all fail.  The cases that exist to
reach a branch (a second grid-stride trip, the G = 4 path with several groups, the n & 7 tail, ragged 32 x 32 pack tiles) assert
from the launch arithmetic that they do."""
import ctypes

import pytest
import torch

from helpers import BF, ERR_INVALID, F32, U8, cdiv, gin, gout, last_error
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
G = 64
CAP = 4096 * 256                        # threads of the largest grid (grid_for in layout.hip)
F16 = torch.float16
DTYPES = {F32: _C.TOK_F32, F16: _C.TOK_F16, BF: _C.TOK_BF16}
# fp32 values a cast can get wrong: half way between two bf16 values (ties go to the even one: down at 1 + 2^-8, up at
# 1 + 3 2^-8), just off the tie on either side, the largest bf16, the first value that rounds to inf, FLT_MAX, signed zeros
SPECIAL = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23,
           3.3895313892515355e38, 3.3961775292304601e38, -3.3961775292304601e38, 3.4028234663852886e38, 0.0, -0.0, 2.0 ** -126]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _run(fn, *args):
    _C.check(getattr(_C.lib(), fn)(*args, stream_ptr()), fn)
    torch.cuda.synchronize()


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(v) * p for v, p in zip(key, (1, 131, 17, 7, 3, 1009, 31, 11))) & 0x7fffffff)


def _values(numel, dtype, g):
    """reals with the special values spread through them (fp32: ties and overflow; fp16: ties, its largest value)"""
    x = torch.randn(numel, generator=g)
    if dtype == F32:
        sp = torch.tensor(SPECIAL, dtype=F32)
    elif dtype == F16:
        sp = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 65504.0, -65504.0, 0.0, -0.0])
    else:
        sp = torch.tensor([3.3895313892515355e38, 0.0, -0.0])
    pos = torch.randperm(numel, generator=g)[:min(numel, 4 * len(sp))]
    x[pos] = sp.repeat(4)[:len(pos)]
    return x.to(dtype)


def test_special_values_are_what_they_claim():
    """(host arithmetic only) the tie values sit half way, the overflow value is past the bf16 maximum"""
    t = torch.tensor(SPECIAL, dtype=F32)
    assert torch.equal(t.double(), torch.tensor(SPECIAL, dtype=torch.float64))            # all exact in fp32
    b = t.to(BF).double()
    assert b[0] == 1.0 and b[1] == 1 + 2.0 ** -6 and b[3] == 1 + 2.0 ** -7 and b[4] == 1.0
    assert torch.isfinite(b[5]) and torch.isinf(b[6]) and torch.isinf(b[7]) and torch.isinf(b[8])


# ---- image NCHW -> NHWC bf16 ---------------------------------------------------------------------------------------------------
NCHW_CASES = [(n, c, cp, h, w) for (c, cp) in ((3, 4), (3, 8), (1, 12), (18, 24), (64, 64)) for (n, h, w) in ((2, 1, 1), (2, 9, 11))]
NCHW_BIG = (3, 3, 4, 600, 600)


@pytest.mark.parametrize('dtype', list(DTYPES), ids=str)
@pytest.mark.parametrize('case', NCHW_CASES + [NCHW_BIG], ids=str)
def test_nchw_to_nhwc(case, dtype):
    n, c, c_pad, h, w = case
    group = 8 if c_pad % 8 == 0 else 4
    if case == NCHW_BIG:
        assert n * h * w * (c_pad // group) > CAP                               # a second grid-stride trip
    if (c, c_pad) == (1, 12):
        assert group == 4 and c_pad // group == 3                               # the G = 4 path with three groups
    x = _values(n * c * h * w, dtype, _gen(*case)).view(n, c, h, w)
    src = gin(x, G)
    dst = gout(n * h * w * c_pad, BF, G)
    _run('tok_nchw_to_nhwc_bf16', src.ptr, DTYPES[dtype], n, c, h, w, dst.ptr, c_pad)
    dst.check(str(case))
    want = torch.zeros(n, h, w, c_pad, dtype=BF)                                # pad channels +0
    want[..., :c] = x.permute(0, 2, 3, 1).to(BF)
    assert torch.equal(_bits(dst.value().view(n, h, w, c_pad)), _bits(want))


# ---- casts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('count', [1, 255, 257, CAP + 17])
def test_cast_f32_bf16(count):
    x = _values(count, F32, _gen(count, 1))
    if count > 1:
        x[count // 2] = float('nan')
    else:
        x[0] = SPECIAL[0]
    src, dst = gin(x, G), gout(count, BF, G)
    _run('tok_cast_f32_bf16', src.ptr, dst.ptr, count)
    dst.check(f'count={count}')
    got, want = dst.value(), x.to(BF)
    assert torch.equal(got.isnan(), want.isnan()) and int(want.isnan().sum()) == (count > 1)       # NaN stays NaN
    ok = ~want.isnan()
    assert torch.equal(_bits(got[ok]), _bits(want[ok]))


@pytest.mark.parametrize('scale', [1.0, 0.125, 1.0 / 3.0])
@pytest.mark.parametrize('count', [1, 7, 8, 9, 1031, 8 * CAP + 13])
def test_cast_bf16_f32(count, scale):
    assert (count & 7 != 0) == (count in (1, 7, 9, 1031, 8 * CAP + 13))          # the tail branch; 8 alone has none
    if count > 8 * CAP:
        assert count // 8 > CAP                                                   # a second grid-stride trip of the 16-byte body
    x = torch.randn(count, generator=_gen(count, 2)).to(BF)
    src, dst = gin(x, G), gout(count, F32, G)
    _run('tok_cast_bf16_f32', src.ptr, dst.ptr, scale, count)
    dst.check(f'count={count} scale={scale}')                                     # the guard right behind an odd count
    want = x.float() * torch.tensor(scale, dtype=F32)                             # one fp32 multiply
    assert torch.equal(dst.value().view(torch.int32), want.view(torch.int32))


# ---- stride-2 subsample (what tests/test_subsample_gpu.py lacks: guards, h = 1, w = 1, a shape past the cap) -----------------------
SUB_BIG = (5, 57, 57, 2048)


@pytest.mark.parametrize('shape', [(2, 1, 1, 8), (2, 1, 6, 8), (3, 5, 1, 16), (1, 1, 7, 24), (2, 4, 6, 8), (2, 5, 7, 8), SUB_BIG], ids=str)
def test_subsample2(shape):
    n, h, w, c = shape
    p, q = (h + 1) // 2, (w + 1) // 2
    if shape == SUB_BIG:
        assert n * p * q * c // 8 > CAP and n * h * w * c // 8 > CAP
    g = _gen(*shape)
    x = torch.randint(-4, 5, shape, generator=g).to(BF)
    src, out = gin(x, G), gout(n * p * q * c, BF, G)
    _run('tok_subsample2_fwd', src.ptr, n, h, w, c, out.ptr)
    out.check(f'fwd {shape}')
    assert torch.equal(_bits(out.value().view(n, p, q, c)), _bits(x[:, ::2, ::2]))
    for integers in (True, False):
        for accumulate in (0, 1):
            if integers:
                dsub, prev = torch.randint(-4, 5, (n, p, q, c), generator=g).to(BF), torch.randint(-4, 5, shape, generator=g).to(BF)
            else:
                dsub, prev = torch.randn(n, p, q, c, generator=g).to(BF), torch.randn(shape, generator=g).to(BF)
            ds = gin(dsub, G)
            dx = gout(n * h * w * c, BF, G, init=prev.cuda() if accumulate else None)
            _run('tok_subsample2_bwd', ds.ptr, n, h, w, c, dx.ptr, accumulate)
            what = f'bwd {shape} integers={integers} accumulate={accumulate}'
            dx.check(what)
            want = prev.clone() if accumulate else torch.zeros(shape, dtype=BF)
            want[:, ::2, ::2] = (want[:, ::2, ::2].float() + dsub.float()).to(BF)       # one fp32 addition, one rounding
            if integers and accumulate:
                assert torch.equal(want.double()[:, ::2, ::2], prev.double()[:, ::2, ::2] + dsub.double())       # exact
            assert torch.equal(_bits(dx.value().view(shape)), _bits(want)), what


# ---- weight packs ------------------------------------------------------------------------------------------------------------------
PACK_SHAPES = [(10, 3, 3, 3, 16, 8, 4), (64, 7, 7, 3, 64, 8, 4), (18, 3, 3, 18, 24, 3, 24), (1000, 1, 1, 2048, 1000, 1, 2048),
               (512, 3, 3, 256, 512, 3, 256)]


def _weight(k, r, s, c, seed):
    g = _gen(k, r, s, c, seed)
    w = torch.randn(k * r * s * c, generator=g)
    w[torch.randperm(w.numel(), generator=g)[:min(w.numel(), len(SPECIAL))]] = torch.tensor(SPECIAL)[:min(w.numel(), len(SPECIAL))]
    return w.view(k, r, s, c)


def _pack_fwd_ref(w, k_pad, s_pad, c_pad):
    k, r, s, c = w.shape
    out = torch.zeros(k_pad, r, s_pad, c_pad, dtype=BF)
    out[:k, :, :s, :c] = w.to(BF)
    return out


def _pack_dgrad_ref(w, k_pad, c_pad):
    """dst[c][r'][s'][k] = src[k][R - 1 - r'][S - 1 - s'][c]"""
    k, r, s, c = w.shape
    out = torch.zeros(c_pad, r, s, k_pad, dtype=BF)
    out[:c, :, :, :k] = w.flip(1, 2).permute(3, 1, 2, 0).to(BF)
    return out


@pytest.mark.parametrize('shape', PACK_SHAPES, ids=str)
def test_pack_weight_single_and_both(shape):
    k, r, s, c, kp, sp, cp = shape
    nf, nd = kp * r * sp * cp, cp * r * s * kp
    if shape == PACK_SHAPES[-1]:
        assert nf > CAP and nd > CAP                                              # a second grid-stride trip in all three kernels
    w = _weight(k, r, s, c, 0)
    src = gin(w, G)
    want_f, want_d = _pack_fwd_ref(w, kp, sp, cp), _pack_dgrad_ref(w, kp, cp)
    f1, d1, f2, d2 = gout(nf, BF, G), gout(nd, BF, G), gout(nf, BF, G), gout(nd, BF, G)
    _run('tok_pack_weight_fwd', src.ptr, k, r, s, c, f1.ptr, kp, sp, cp)
    _run('tok_pack_weight_dgrad', src.ptr, k, r, s, c, d1.ptr, kp, cp)
    _run('tok_pack_weight_both', src.ptr, k, r, s, c, f2.ptr, kp, sp, cp, d2.ptr)
    for name, buf, want in (('fwd', f1, want_f), ('dgrad', d1, want_d), ('both/fwd', f2, want_f), ('both/dgrad', d2, want_d)):
        buf.check(f'{name} {shape}')
        assert torch.equal(_bits(buf.value()), _bits(want.reshape(-1))), f'{name} {shape}'
    assert torch.equal(_bits(f1.value()), _bits(f2.value())) and torch.equal(_bits(d1.value()), _bits(d2.value()))


BATCH_ITEMS = [  # (k, r, s, c, k_pad, s_pad, c_pad), which destinations
    ((10, 3, 3, 3, 16, 8, 4), 'both'), ((64, 7, 7, 3, 64, 8, 4), 'fwd'), ((18, 3, 3, 18, 24, 3, 24), 'both'),
    ((18, 3, 3, 33, 24, 3, 40), 'both'), ((1000, 1, 1, 2048, 1000, 1, 2048), 'dgrad'), ((19, 1, 1, 40, 24, 1, 40), 'both'),
    ((512, 3, 3, 256, 512, 3, 256), 'both')]


def _batched(items_spec, seed):
    lib = _C.lib()
    items, keep, block = [], [], 0
    for i, (shape, which) in enumerate(items_spec):
        k, r, s, c, kp, sp, cp = shape
        w = _weight(k, r, s, c, seed + i)
        src = gin(w, G)
        f = gout(kp * r * sp * cp, BF, G) if which in ('both', 'fwd') else None
        d = gout(cp * r * s * kp, BF, G) if which in ('both', 'dgrad') else None
        it = _C.PackItem(src.ptr, f.ptr if f else None, d.ptr if d else None, k, r, s, c, kp, sp, cp, block)
        blocks = lib.tok_pack_item_blocks(ctypes.byref(it))
        assert blocks == cdiv(kp, 32) * cdiv(cp, 32) * r * sp, shape             # one block per 32 x 32 tile of every stored tap
        block += blocks
        items.append(it)
        keep.append((shape, w, src, f, d))
    table = gin(torch.frombuffer(bytearray(bytes((_C.PackItem * len(items))(*items))), dtype=U8), 256)
    _run('tok_pack_weights_batched', table.ptr, len(items), block)
    for shape, w, src, f, d in keep:
        k, r, s, c, kp, sp, cp = shape
        if f is not None:
            f.check(f'batched fwd {shape}')
            assert torch.equal(_bits(f.value()), _bits(_pack_fwd_ref(w, kp, sp, cp).reshape(-1))), f'batched fwd {shape}'
        if d is not None:
            d.check(f'batched dgrad {shape}')
            assert torch.equal(_bits(d.value()), _bits(_pack_dgrad_ref(w, kp, cp).reshape(-1))), f'batched dgrad {shape}'
            # and bit for bit the single pack of the device
            d1 = gout(cp * r * s * kp, BF, G)
            _run('tok_pack_weight_dgrad', src.ptr, k, r, s, c, d1.ptr, kp, cp)
            assert torch.equal(_bits(d.value()), _bits(d1.value()))
        if f is not None:
            f1 = gout(kp * r * sp * cp, BF, G)
            _run('tok_pack_weight_fwd', src.ptr, k, r, s, c, f1.ptr, kp, sp, cp)
            assert torch.equal(_bits(f.value()), _bits(f1.value()))


def test_pack_weights_batched():
    shapes = [s for s, _ in BATCH_ITEMS]
    assert len(BATCH_ITEMS) >= 6 and any(s[4] % 32 and s[6] % 32 and s[6] > 32 for s in shapes)      # ragged tiles in k and in c
    assert (18, 3, 3, 33, 24, 3, 40) in shapes and any(s[5] > s[2] for s in shapes)                  # k_pad 24, c_pad 40; s_pad > s
    assert {w for _, w in BATCH_ITEMS} == {'both', 'fwd', 'dgrad'}                                   # a NULL dst_dgrad, a NULL dst_fwd
    _batched(BATCH_ITEMS, 0)


@pytest.mark.parametrize('item', [BATCH_ITEMS[0], BATCH_ITEMS[3]], ids=str)
def test_pack_weights_batched_single_item_table(item):
    _batched([item], 50)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """every TOK_CHECK_ARG of layout.hip: the invalid-argument code, the function named in tok_last_error, nothing written"""
    lib, st = _C.lib(), stream_ptr()
    src = gin(torch.zeros(4096), G)
    out, outf = gout(4096, BF, G), gout(4096, F32, G)
    i, o, f = src.ptr, out.ptr, outf.ptr
    calls = [('tok_nchw_to_nhwc_bf16', (None, 0, 1, 3, 4, 4, o, 4, st)), ('tok_nchw_to_nhwc_bf16', (i, 0, 1, 3, 4, 4, None, 4, st))]
    for n, c, h, w, cp, dt in ((0, 3, 4, 4, 4, 0), (1, 0, 4, 4, 4, 0), (1, 3, 0, 4, 4, 0), (1, 3, 4, -1, 4, 0), (1, 5, 4, 4, 4, 0),
                               (1, 3, 4, 4, 6, 0), (1, 3, 4, 4, 0, 0), (1, 3, 4, 4, 4, 3), (1, 3, 4, 4, 4, -1)):
        calls.append(('tok_nchw_to_nhwc_bf16', (i, dt, n, c, h, w, o, cp, st)))      # sizes, c_pad < c, c_pad % 4, unknown dtype
    calls += [('tok_cast_f32_bf16', (None, o, 8, st)), ('tok_cast_f32_bf16', (i, None, 8, st)), ('tok_cast_f32_bf16', (i, o, 0, st)),
              ('tok_cast_bf16_f32', (None, f, 1.0, 8, st)), ('tok_cast_bf16_f32', (i, None, 1.0, 8, st)),
              ('tok_cast_bf16_f32', (i, f, 1.0, 0, st)), ('tok_cast_bf16_f32', (i + 2, f, 1.0, 8, st)),
              ('tok_cast_bf16_f32', (i, f + 4, 1.0, 8, st))]                          # misaligned source, misaligned destination
    for n, h, w, c in ((0, 4, 4, 8), (1, 0, 4, 8), (1, 4, 0, 8), (1, 4, 4, 0), (1, 4, 4, 12)):
        calls += [('tok_subsample2_fwd', (i, n, h, w, c, o, st)), ('tok_subsample2_bwd', (i, n, h, w, c, o, 0, st))]
    calls += [('tok_subsample2_fwd', (None, 1, 4, 4, 8, o, st)), ('tok_subsample2_fwd', (i, 1, 4, 4, 8, None, st)),
              ('tok_subsample2_bwd', (None, 1, 4, 4, 8, o, 0, st)), ('tok_subsample2_bwd', (i, 1, 4, 4, 8, None, 0, st))]
    ok = dict(k=4, r=3, s=3, c=4, kp=8, sp=4, cp=8)
    for bad in (dict(k=0), dict(r=0), dict(s=0), dict(c=-1), dict(kp=3), dict(sp=2), dict(cp=3), dict(src=None), dict(dst=None)):
        a = dict(ok, **{k: v for k, v in bad.items() if k not in ('src', 'dst')})
        sp_, dp_ = (None if 'src' in bad else i), (None if 'dst' in bad else o)
        calls.append(('tok_pack_weight_fwd', (sp_, a['k'], a['r'], a['s'], a['c'], dp_, a['kp'], a['sp'], a['cp'], st)))
        calls.append(('tok_pack_weight_both', (sp_, a['k'], a['r'], a['s'], a['c'], dp_, a['kp'], a['sp'], a['cp'], o, st)))
        if 'sp' not in bad:
            calls.append(('tok_pack_weight_dgrad', (sp_, a['k'], a['r'], a['s'], a['c'], dp_, a['kp'], a['cp'], st)))
    calls += [('tok_pack_weight_both', (i, 4, 3, 3, 4, o, 8, 4, 8, None, st)),
              ('tok_pack_weights_batched', (None, 1, 1, st)), ('tok_pack_weights_batched', (i, 0, 1, st)),
              ('tok_pack_weights_batched', (i, 1, 0, st))]
    for fn, args in calls:
        rc = getattr(lib, fn)(*args)
        assert rc == ERR_INVALID and fn + ':' in last_error(), (fn, args[:-1], rc, last_error())
    assert lib.tok_pack_item_blocks(None) == 0
    torch.cuda.synchronize()
    for buf in (out, outf):
        buf.check('refused call')
        assert buf.untouched()
    src.check('refused call')
