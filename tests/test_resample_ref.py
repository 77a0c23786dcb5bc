"""The fp64 reference of the resample contract modules (tests/resample_ref.py) against torch itself, on the CPU.

up64 against F.interpolate(x.double(), mode='bilinear', align_corners=False): ATen evaluates the scale of a double tensor in
fp64, the reference rounds the quotient to fp32 once (its definition), so the two source coordinates differ by at most
2^-24 scale (d + 0.5) <= 2^-24 (s + 1) = d lam / K_LAM, and the results by that times the local slope — lam_term / K_LAM —
plus fp64 roundoff (1e-14 of the magnitude).  The transpose alike against autograd, with lam_term_T.  The fuse sum against its
definition written with repeat_interleave, exactly."""
import pytest
import torch
import torch.nn.functional as F

import resample_ref as R
from helpers import BF, assert_bounded, pack_bits, unpack_bits

SIZES = [((1, 1), (2, 2)), ((8, 8), (16, 16)), ((2, 4), (16, 32)), ((5, 7), (13, 20)), ((7, 5), (7, 10)), ((9, 9), (4, 5)),
         ((3, 3), (1, 1)), ((8, 8), (8, 8)), ((11, 11), (32, 32)), ((3, 3), (24, 24))]
_ids = lambda v: 'x'.join(str(i) for t in v for i in t)      # noqa: E731


def _interp(x, size, **kw):
    return F.interpolate(x.permute(0, 3, 1, 2), size=size, mode='bilinear', **kw).permute(0, 2, 3, 1)


@pytest.mark.parametrize('size', SIZES, ids=_ids)
def test_source_index_definition(size):
    for n_in, n_out in zip(*size):
        i0, i1, lam, dlam = R.src_index(n_in, n_out)
        assert i0.shape == (n_out,) and int(i0.min()) >= 0 and int(i1.max()) <= n_in - 1
        assert bool(((i1 == i0) | (i1 == i0 + 1)).all()) and bool((i1[i0 < n_in - 1] == i0[i0 < n_in - 1] + 1).all())
        assert bool((lam >= 0).all()) and bool((lam < 1).all()) and bool((dlam >= R.K_LAM * R.U32).all())
        w = R.weight_matrix(n_in, n_out)
        assert torch.allclose(w.sum(1), torch.ones(n_out, dtype=torch.float64), rtol=0, atol=1e-15)
        if R.dyadic(n_in, n_out):       # multiples of 1 / (2 factor): exact in fp32 (and in bf16 up to factor 64)
            assert torch.equal(w * 2 * (n_out // n_in), (w * 2 * (n_out // n_in)).round())
        # the footprint count is the densest column of W
        assert R.taps_T(n_in, n_out) == int((w > 0).sum(0).max())


@pytest.mark.parametrize('size', SIZES, ids=_ids)
def test_up64_is_aten_bilinear(size):
    (hs, ws), (hd, wd) = size
    g = torch.Generator().manual_seed(hs * 31 + wd)
    x = torch.randn(2, hs, ws, 5, generator=g).to(BF)
    ref, mag = R.up64(x, (hd, wd)), R.up_mag(x, (hd, wd))
    aten = _interp(x.double(), (hd, wd), align_corners=False)
    assert_bounded(aten, ref, R.lam_term(x, (hd, wd)) / R.K_LAM + 1e-14 * mag, 0.0, 1.0, 'up64 against ATen in fp64')
    assert torch.equal(R.up64(x, (hd, wd), rows=(hd // 2, hd)), ref[:, hd // 2:])
    # ATen's fp32 path is one evaluation the contract's bound has to hold for: s in fp32, two rounded weights per axis, four
    # roundings of the blend (b = 7 2^-24, derived in tests/test_resample_contract_gpu.py) — and no bf16 rounding here (a = 0)
    fp32 = _interp(x.float(), (hd, wd), align_corners=False)
    assert_bounded(fp32, ref, 7 * R.U32 * mag + R.lam_term(x, (hd, wd)), 0.0, 1.0, 'up64 against ATen in fp32')
    if (hs, ws) != (hd, wd) and min(hs, ws) > 1:        # ... and not for another sampling grid
        with pytest.raises(AssertionError):
            assert_bounded(_interp(x.float(), (hd, wd), align_corners=True), ref, 7 * R.U32 * mag + R.lam_term(x, (hd, wd)), 2.0 ** -8, 1.0)


@pytest.mark.parametrize('size', SIZES, ids=_ids)
def test_up64_T_is_the_autograd_transpose(size):
    (hs, ws), (hd, wd) = size
    g = torch.Generator().manual_seed(hs * 37 + wd)
    grad = torch.randn(2, hd, wd, 5, generator=g).to(BF)
    x = torch.zeros(2, hs, ws, 5, dtype=torch.float64, requires_grad=True)
    _interp(x, (hd, wd), align_corners=False).backward(grad.double())
    ref, mag = R.up64_T(grad, (hs, ws)), R.up_T_mag(grad, (hs, ws))
    assert_bounded(x.grad, ref, R.lam_term_T(grad, (hs, ws)) / R.K_LAM + 1e-14 * mag, 0.0, 1.0, 'up64_T against autograd')
    # the transpose, as a matrix identity in fp64: <up(x), g> = <x, up^T(g)>
    xr = torch.randn(2, hs, ws, 5, generator=g, dtype=torch.float64)
    a, b = float((R.up64(xr, (hd, wd)) * grad.double()).sum()), float((xr * ref).sum())
    assert abs(a - b) <= 1e-12 * float((R.up_mag(xr, (hd, wd)) * grad.double().abs()).sum())
    # and through the dense per-axis matrices the lam terms are built from
    wy, wx = R.weight_matrix(hs, hd), R.weight_matrix(ws, wd)
    assert torch.allclose(torch.einsum('da,ndec,eb->nabc', wy, grad.double(), wx), ref, rtol=0, atol=1e-13)


def test_footprints():
    assert [R.taps_T(64 // f, 64) for f in (1, 2, 4, 8)] == [1, 4, 8, 16]          # 2F destinations per interior source and axis
    assert R.taps_T(2, 16) == 12                                                      # a border source: F / 2 clamped + F
    assert R.dyadic(8, 8) and R.dyadic(1, 2) and R.dyadic(2, 16) and not R.dyadic(5, 13) and not R.dyadic(9, 4) and not R.dyadic(4, 12)


@pytest.mark.parametrize('n,h,w,c,shifts', [(2, 16, 16, 16, (0, 1, 2, 3)), (2, 8, 24, 48, (0, 0, 1)), (1, 8, 8, 8, (0,)), (3, 8, 8, 64, (0, 2))])
@pytest.mark.parametrize('relu', (0, 1))
def test_fuse64_is_the_definition(n, h, w, c, shifts, relu):
    g = torch.Generator().manual_seed(h + c + relu)
    terms = [torch.randn(n, h >> s, w >> s, c, generator=g).to(BF) for s in shifts]
    scs = [torch.rand(c, generator=g) + 0.5 if j % 2 == 0 else None for j in range(len(shifts))]
    sfs = [torch.randn(c, generator=g) if j % 2 == 0 else None for j in range(len(shifts))]
    want = torch.zeros(n, h, w, c, dtype=torch.float64)
    for t, s, sc, sf in zip(terms, shifts, scs, sfs):
        v = t.double() if sc is None else t.double() * sc.double() + sf.double()
        want = want + v.repeat_interleave(1 << s, dim=1).repeat_interleave(1 << s, dim=2)
    if relu:
        want = want.clamp_min(0)
    got = R.fuse64(terms, shifts, scs, sfs, relu)
    assert torch.equal(got, want)
    assert bool((R.fuse64(terms, shifts, scs, sfs, relu, absolute=True) >= got.abs()).all())
    stored = got.to(BF)
    mask = R.fuse_mask(stored)
    assert mask.shape == (n * h * w, c // 8) and torch.equal(unpack_bits(mask, n * h * w, c), (stored.float() > 0).view(-1, c))
    assert torch.equal(mask, pack_bits((stored.float() > 0).view(-1, c)))
    # backward: autograd of the same definition
    grad = torch.randn(n, h, w, c, generator=g).to(BF)
    keep = stored.float() > 0
    for j, s in enumerate(shifts):
        t = terms[j].double().requires_grad_(True)
        up = t.repeat_interleave(1 << s, dim=1).repeat_interleave(1 << s, dim=2)
        (up * torch.where(keep, grad.double(), torch.zeros((), dtype=torch.float64))).sum().backward()
        prev = torch.randn(n, h >> s, w >> s, c, generator=g).to(BF)
        assert torch.allclose(R.fuse_T64(grad, keep, s), t.grad, rtol=0, atol=1e-12)
        assert torch.allclose(R.fuse_T64(grad, keep, s, prev), t.grad + prev.double(), rtol=0, atol=1e-12)
        assert torch.allclose(R.fuse_T64(grad, None, s), grad.double().view(n, h >> s, 1 << s, w >> s, 1 << s, c).sum((2, 4)), rtol=0, atol=1e-12)
