"""The gradient-clip kernels (csrc/grad_clip.hip: tok_grad_sqnorm_partial, tok_grad_clip_coef, tok_grad_scale, tok_grad_clamp) on span
tables built directly (int64 [n][3] = tok_grad_span: grad pointer, numel, start, as torchok_amd/optim/clip.py packs them); the
references, their bounds and the span lists are in tests/unit3_clip_ref.py (tests/test_unit3_clip_ref.py holds them to
torch.nn.utils.clip_grad_norm_ / clip_grad_value_).

All spans of a list live in ONE guarded arena, each slot on a 256-byte boundary; the padding between the slots and a stale slot that
is in no span hold NaN (a payload of their own) and must keep their bits after every launch, as must the guards.  Every fp64 partial
is compared with the sum of squares of its own slice of the span space; exactly `grid` partials are written, those behind keep their
sentinel (the list `zero_block` has a block whose slice is all zero: it writes 0.0).  total_norm and coef are bit-equal to the fp32 restatement of include/tok.h (the fold in the kernel's order); scale is
bit-exact against the fp32 product with the stored coef, clamp against torch.clamp_.  Every launch runs twice from the same state and
must give the same bits.

Exclusions, named: where x * coef is NaN (x NaN, coef NaN, inf * 0) only NaN-ness is compared, not the payload (IEEE leaves it open);
a NaN under clamp, and every element under coef = 1, keeps its own bits exactly."""
import numpy as np
import pytest
import torch

from helpers import ERR_INVALID, F32, cdiv, gin, gout, last_error
import unit3_clip_ref as M
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
TAG = 'unit3_clip_contract/'
I32, I64 = torch.int32, torch.int64
PAD_NAN = 0x7FC00ABC                 # the padding and the stale slot
PLANTED_NAN = 0x7FC12345              # a NaN planted inside a span


@pytest.fixture(autouse=True, scope='module')
def _parity_record():
    yield
    M.flush_record()


def ok(rc, what):
    _C.check(rc, what)
    torch.cuda.synchronize()


class Arena:
    """the spans of one list in a guarded arena: slot i at a 256-byte boundary, a stale slot (64 floats, in no span) after the second
    span, NaN everywhere outside the spans; `table`: the device span table behind NaN guards"""

    def __init__(self, vals):
        self.vals = vals
        offs, o = [], 0
        for i, v in enumerate(vals):
            offs.append(o)
            o += cdiv(v.numel(), 64) * 64
            if i == 1:
                o += 64
        self.offs, self.numel, self.total = offs, o + 64, sum(v.numel() for v in vals)
        host = torch.full((self.numel,), PAD_NAN, dtype=I32)
        self.owned = torch.zeros(self.numel, dtype=torch.bool)
        for off, v in zip(offs, vals):
            host[off:off + v.numel()] = v.view(I32)
            self.owned[off:off + v.numel()] = True
        self.host = host
        self.span = gout(self.numel, F32, 1024)
        self.reset()
        base = self.span.ptr
        assert base % 256 == 0
        rows, start = [], 0
        for off, v in zip(offs, vals):
            rows.append((base + 4 * off, v.numel(), start))
            start += v.numel()
        self.table = gin(torch.tensor(rows, dtype=I64).reshape(-1).cuda(), 64)
        self.n = len(vals)

    def reset(self):
        self.span.view.view(I32).copy_(self.host.cuda())

    def bits(self):
        """the arena's bits on the host, after checking the guards, the padding and the stale slot"""
        self.span.check('arena')
        self.table.check('span table')
        iv = self.span.view.view(I32).cpu()
        assert bool((iv[~self.owned] == PAD_NAN).all()), 'padding or the stale slot written'
        return iv

    def spans(self, iv):
        return [iv[o:o + v.numel()].view(F32) for o, v in zip(self.offs, self.vals)]


def partials_buf(fill=None):
    s = gout(M.MAX_PARTIALS, I64, 64)
    if fill is not None:
        s.view[:len(fill)].view(torch.float64).copy_(torch.tensor(fill, dtype=torch.float64))
    return s


def sqnorm(a):
    lib, st = _C.lib(), stream_ptr()
    grid = M.clip_grid(a.total)
    out = []
    for _ in range(2):
        pb = partials_buf()
        ok(lib.tok_grad_sqnorm_partial(a.table.ptr, a.n, a.total, pb.ptr, st), 'sqnorm_partial')
        pb.check('partials')
        unwritten = pb.view == pb.bits
        assert not bool(unwritten[:grid].any()) and bool(unwritten[grid:].all()), 'the partials written are not exactly the first `grid`'
        out.append(pb)
    assert torch.equal(out[0].buf, out[1].buf), 'two runs differ'
    assert torch.equal(a.bits(), a.host), 'the norm pass wrote to the arena'
    return out[0]


def coef_of(pb, total, max_norm):
    lib, st = _C.lib(), stream_ptr()
    res = []
    for _ in range(2):
        sc = gout(2, F32, 64)
        ok(lib.tok_grad_clip_coef(pb.ptr, total, max_norm, sc.ptr, sc.ptr + 4, st), 'clip_coef')
        sc.check('scalars')
        res.append(sc)
    assert torch.equal(res[0].buf.view(I32), res[1].buf.view(I32))
    pb.check('partials')
    return res[0]


def check_coef(pb, total, max_norm):
    sc = coef_of(pb, total, max_norm)
    part = pb.view[:M.clip_grid(total)].view(torch.float64).cpu().numpy()
    tot, c = M.clip_coef_f32(part, max_norm)
    got = sc.value().numpy()
    want = np.array([tot, c], dtype=np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)) or (np.isnan(want).all() and np.isnan(got).all()), (got, want)
    return sc, float(tot), float(c)


def scale_with(a, coef_ptr):
    lib, st = _C.lib(), stream_ptr()
    res = []
    for _ in range(2):
        a.reset()
        ok(lib.tok_grad_scale(a.table.ptr, a.n, a.total, coef_ptr, st), 'grad_scale')
        res.append(a.bits())
    assert torch.equal(res[0], res[1]), 'two runs differ'
    return a.spans(res[0])


def clamp_with(a, v):
    lib, st = _C.lib(), stream_ptr()
    res = []
    for _ in range(2):
        a.reset()
        ok(lib.tok_grad_clamp(a.table.ptr, a.n, a.total, v, st), 'grad_clamp')
        res.append(a.bits())
    assert torch.equal(res[0], res[1]), 'two runs differ'
    return a.spans(res[0])


def same_or_nan(got, want, what):
    """bit-equal, except where the reference is NaN: there NaN-ness only (the payload of a computed NaN is left open)"""
    for i, (g, w) in enumerate(zip(got, want)):
        nan = torch.isnan(w)
        assert bool(torch.isnan(g[nan]).all()), f'{what}: span {i} lost a NaN'
        assert torch.equal(g[~nan].view(I32), w[~nan].view(I32)), f'{what}: span {i} differs'


@pytest.mark.parametrize('name', list(M.SPAN_LISTS))
def test_grad_clip_span_list(name):
    """partials per slice, the norm and coefficient for max_norm below and above the norm, the scale by the stored coefficient,
    the clamp: every cut of a slice or a span inside a 4-element group is in one of the lists"""
    vals = M.make_spans(M.SPAN_LISTS[name])
    a = Arena(vals)
    total, grid = a.total, M.clip_grid(a.total)
    pb = sqnorm(a)
    ref, bnd = M.grad_partials_ref(vals)
    M.check(TAG + 'grad_sqnorm_partial', 'partials', pb.view[:grid].view(torch.float64).cpu(), ref, bnd)
    exact = M.math_norm(vals)
    for max_norm in (0.5 * exact, 2.0 * exact):
        sc, tot, c = check_coef(pb, total, max_norm)
        assert abs(tot - exact) <= 1.01 * 2.0 ** -24 * exact
        assert (c == 1.0) == (max_norm > exact)
        got = scale_with(a, sc.ptr + 4)
        same_or_nan(got, M.grad_scale_ref(vals, c), f'scale by {c}')
    v = 0.5 * float(np.median(np.abs(np.concatenate([t.numpy() for t in vals]))))
    got = clamp_with(a, v)
    same_or_nan(got, M.grad_clamp_ref(vals, v), 'clamp')
    assert any(bool((t.abs() > v).any()) for t in vals)


def _with_specials(numels, seed=3):
    vals = M.make_spans(numels, seed)
    sp = torch.tensor([float('inf'), float('-inf'), 0.0, -0.0, 1e-3, -1e-3, 1e-45, -1e-45, 3e38, -3e38])
    big = max(range(len(vals)), key=lambda i: vals[i].numel())
    vals[big][:sp.numel()] = sp
    vals[big][-sp.numel():] = sp.flip(0)
    vals[big].view(I32)[sp.numel()] = PLANTED_NAN
    vals[big].view(I32)[-sp.numel() - 1] = PLANTED_NAN
    for v in vals:
        if v.numel() < 4:
            v.view(I32)[0] = PLANTED_NAN
            break
    return vals


@pytest.mark.parametrize('coef', [1.0, 0.5, 0.0, float('nan')])
@pytest.mark.parametrize('name', ['mixed', 'cut_in_group'])
def test_grad_scale_coefs(name, coef):
    vals = _with_specials(M.SPAN_LISTS[name])
    a = Arena(vals)
    c = gin(torch.tensor([coef], dtype=F32).cuda(), 64)
    got = scale_with(a, c.ptr)
    c.check('coef')
    if coef == 1.0:
        for g, v in zip(got, vals):
            assert torch.equal(g.view(I32), v.view(I32)), 'coef = 1 changed bits'
    else:
        same_or_nan(got, M.grad_scale_ref(vals, coef), f'scale by {coef}')


@pytest.mark.parametrize('v', [1e-3, 0.0, -1.0, float('inf')])
@pytest.mark.parametrize('name', ['mixed', 'cut_in_group'])
def test_grad_clamp_values(name, v):
    vals = _with_specials(M.SPAN_LISTS[name])
    a = Arena(vals)
    got = clamp_with(a, v)
    want = M.grad_clamp_ref(vals, v)
    for i, (g, w, x) in enumerate(zip(got, want, vals)):
        nan = torch.isnan(x)
        assert bool(torch.isnan(w[nan]).all()) and torch.equal(g[nan].view(I32), x[nan].view(I32)), f'span {i}: a NaN changed'
        assert torch.equal(g[~nan].view(I32), w[~nan].view(I32)), f'span {i} differs from torch.clamp_'


def test_clip_coef_edges():
    """norm 0 (coef = min(max_norm / 1e-6, 1)); a sum of squares beyond fp32 range (norm inf, coef 0); a NaN partial (both NaN); a
    partial count that is no multiple of the block"""
    total = 3 * M.MIN_PER_BLOCK
    for fill, max_norm, want in (([0.0, 0.0, 0.0], 0.5, (0.0, 1.0)),
                                 ([0.0, 0.0, 0.0], 1e-7, (0.0, float(np.float32(1e-7) / np.float32(1e-6)))),
                                 ([1e80, 1e80, 3.0], 1.0, (float('inf'), 0.0)),
                                 ([1.0, float('nan'), 1.0], 1.0, (float('nan'), float('nan')))):
        _, tot, c = check_coef(partials_buf(fill), total, max_norm)
        assert (np.isnan(tot) and np.isnan(c)) if np.isnan(want[0]) else (tot, c) == want, (tot, c, want)
    g = np.random.default_rng(1).random(777) * 1e3
    check_coef(partials_buf(list(g)), 777 * M.MIN_PER_BLOCK, 100.0)


def test_grad_clip_refusals():
    lib, st = _C.lib(), stream_ptr()
    vals = M.make_spans(M.SPAN_LISTS['mixed'])
    a = Arena(vals)
    pb, sc = partials_buf(), gout(2, F32, 64)
    t, n, tot = a.table.ptr, a.n, a.total
    calls = [lambda: lib.tok_grad_sqnorm_partial(None, n, tot, pb.ptr, st), lambda: lib.tok_grad_sqnorm_partial(t, n, tot, None, st),
             lambda: lib.tok_grad_sqnorm_partial(t, 0, tot, pb.ptr, st), lambda: lib.tok_grad_sqnorm_partial(t, -1, tot, pb.ptr, st),
             lambda: lib.tok_grad_sqnorm_partial(t, n, 0, pb.ptr, st), lambda: lib.tok_grad_sqnorm_partial(t, n, -5, pb.ptr, st),
             lambda: lib.tok_grad_clip_coef(None, tot, 1.0, sc.ptr, sc.ptr + 4, st),
             lambda: lib.tok_grad_clip_coef(pb.ptr, tot, 1.0, None, sc.ptr + 4, st),
             lambda: lib.tok_grad_clip_coef(pb.ptr, tot, 1.0, sc.ptr, None, st),
             lambda: lib.tok_grad_clip_coef(pb.ptr, 0, 1.0, sc.ptr, sc.ptr + 4, st),
             lambda: lib.tok_grad_scale(None, n, tot, sc.ptr, st), lambda: lib.tok_grad_scale(t, n, tot, None, st),
             lambda: lib.tok_grad_scale(t, 0, tot, sc.ptr, st), lambda: lib.tok_grad_scale(t, n, 0, sc.ptr, st),
             lambda: lib.tok_grad_clamp(None, n, tot, 1.0, st), lambda: lib.tok_grad_clamp(t, 0, tot, 1.0, st),
             lambda: lib.tok_grad_clamp(t, n, 0, 1.0, st), lambda: lib.tok_grad_clamp(t, n, -1, 1.0, st)]
    for i, call in enumerate(calls):
        rc = call()
        torch.cuda.synchronize()
        assert rc == ERR_INVALID and 'tok_grad_' in last_error(), (i, rc, last_error())
    assert pb.untouched() and sc.untouched()
    pb.check('partials')
    sc.check('scalars')
    assert torch.equal(a.bits(), a.host)
