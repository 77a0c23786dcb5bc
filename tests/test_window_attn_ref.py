"""The fp64 window-attention reference (tests/window_attn_ref.py) against the fake backend's independent restatement
(torch.roll + view partition, fp32), and the reference's own bounds: an emulation of the device's rounding points must stay
inside HALF of every bound of the contract, so an exact kernel provably passes tests/test_window_attn_contract_gpu.py."""
import pytest
import torch

from fake_backend import FakeTok
from helpers import assert_bounded
from window_attn_ref import HD, WinRef, check_result, emulate_device, make_inputs, shift_mask

P = lambda t: None if t is None else t.data_ptr()       # noqa: E731


def _close(mine, want, what, tol=2e-5):
    err = float((mine.double() - want.double()).abs().max())
    assert err <= tol * max(float(want.abs().max()), 1e-30), (what, err, float(want.abs().max()))


@pytest.mark.parametrize('b,h,w,heads,ws,shift,plain', [
    (2, 8, 12, 3, 4, 0, 0), (2, 8, 12, 3, 4, 2, 0), (1, 14, 21, 2, 7, 3, 0), (1, 16, 8, 1, 8, 4, 0), (2, 9, 18, 2, 9, 4, 0),
    (2, 14, 7, 2, 7, 0, 1), (1, 8, 16, 2, 8, 0, 1)])
def test_reference_agrees_with_fake_backend(b, h, w, heads, ws, shift, plain):
    c, n = heads * HD, ws * ws
    qkv, dout, ls, bias, mask = make_inputs(b, h, w, heads, ws, shift, seed=11, plain=bool(plain), ls0=5.0)
    ref = WinRef(qkv, dout, b, h, w, heads, ws, shift, ls, bias, mask, chunk=1)
    fake = FakeTok()
    with torch.enable_grad():
        x, fls, fbi, o, lse = fake._attn(P(qkv), b, h, w, c, heads, ws, shift, 3 * c, P(ls), P(bias), P(mask))
        gx, gls, gbi = torch.autograd.grad(o, (x, fls, fbi), dout.float().view(b, h, w, c))
    _close(o.detach().reshape(-1, c), ref.out, 'out')
    _close(lse.detach().reshape(-1, n), ref.lse, 'lse')
    for i, what in enumerate(('dq', 'dk', 'dv')):
        _close(gx.reshape(-1, 3 * c)[:, i * c:(i + 1) * c], ref.grad[i], what)
    if not plain:
        _close(gbi, ref.dbias, 'dbias')
        _close(gls, ref.dls, 'dlogit_scale')
        assert float(ref.dls[0]) == 0.0 and float(gls[0]) == 0.0          # head 0 is clamped


def test_shift_mask_is_the_swin_mask():
    """the index-table mask against the construction of SwinTransformerBlock (roll-free image of region numbers, view partition)"""
    for h, w, ws, shift in ((8, 12, 4, 2), (14, 21, 7, 3), (16, 8, 8, 4), (9, 18, 9, 4)):
        n = ws * ws
        img = torch.zeros(1, h, w, 1)
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                img[:, hs, wsl, :] = cnt
                cnt += 1
        mw = img.view(1, h // ws, ws, w // ws, ws, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, n)
        am = mw.unsqueeze(1) - mw.unsqueeze(2)
        assert torch.equal(am.masked_fill(am != 0, -100.0).masked_fill(am == 0, 0.0), shift_mask(h, w, ws, shift))


# the shapes of the GPU contract module (multi-image ones at three images: the bounds are per element / per row), N = 16, 49, 64
# on the MFMA path at scales e^2.3 and one head at 100 where the backward gates allow it, N = 81, 256 on the scalar path
EMULATED = [
    dict(b=2, h=8, w=12, heads=3, ws=4, shift=0), dict(b=2, h=8, w=12, heads=3, ws=4, shift=2),
    dict(b=1, h=14, w=21, heads=2, ws=7, shift=3), dict(b=1, h=16, w=8, heads=1, ws=8, shift=4),
    dict(b=3, h=8, w=8, heads=3, ws=4, shift=2), dict(b=3, h=14, w=14, heads=3, ws=7, shift=3),
    dict(b=3, h=14, w=14, heads=3, ws=7, shift=0, plain=True), dict(b=3, h=8, w=8, heads=12, ws=8, shift=0),
    dict(b=3, h=8, w=8, heads=6, ws=4, shift=0),
    dict(b=2, h=9, w=18, heads=2, ws=9, shift=4, ls0=5.0), dict(b=1, h=16, w=32, heads=1, ws=16, shift=8, ls0=5.0),
    dict(b=2, h=8, w=12, heads=3, ws=4, shift=2, sharp_head=1), dict(b=1, h=14, w=21, heads=2, ws=7, shift=3, sharp_head=0),
]


@pytest.mark.parametrize('case', EMULATED, ids=lambda d: '-'.join(f'{k}{v}' for k, v in d.items()))
def test_rounding_emulation_stays_inside_half_of_every_bound(case):
    case = dict(case)
    extra = {k: case.pop(k) for k in ('plain', 'ls0', 'sharp_head', 'ls_mean') if k in case}
    dims = tuple(case[k] for k in ('b', 'h', 'w', 'heads', 'ws', 'shift'))
    bpw = 2 if dims[0] == 3 else 1              # three images: a scratch row of two and a last one of one
    qkv, dout, ls, bias, mask = make_inputs(*dims, seed=5, **extra)
    ref = WinRef(qkv, dout, *dims, ls, bias, mask, bpw=bpw)
    got = emulate_device(qkv, dout, *dims, ls, bias, mask, bpw=bpw)
    check_result('emulation', ref, *got, frac=0.5, record=False)


@pytest.mark.parametrize('dims,bpw', [((2, 8, 12, 3, 4, 2), 1), ((1, 16, 8, 1, 8, 4), 1), ((16, 14, 14, 3, 7, 3), 1),
                                      ((33, 8, 8, 3, 4, 2), 16), ((2, 9, 18, 2, 9, 4), 1)])
def test_wrong_parameter_gradients_fail_the_contract(dims, bpw):
    """what the envelopes alone let through: a zero, doubled or sign-flipped d(logit_scale), 0.9 d(bias) spread over the
    scratch rows, and a last scratch row that lacks its last image (1 of 33 images here)"""
    qkv, dout, ls, bias, mask = make_inputs(*dims, seed=9)
    ref = WinRef(qkv, dout, *dims, ls, bias, mask, bpw=bpw)
    out, lse, dqkv, dbias, dls, scr, part = emulate_device(qkv, dout, *dims, ls, bias, mask, bpw=bpw)
    check_result('emulation', ref, out, lse, dqkv, dbias, dls, scr, part, record=False)
    for f in (0.0, 2.0, -1.0):
        with pytest.raises(AssertionError):
            check_result('wrong', ref, out, lse, dqkv, dbias, f * dls, scr, f * part, record=False)
        with pytest.raises(AssertionError):
            check_result('wrong', ref, out, lse, dqkv, dbias, f * dls, record=False)          # ... on the total alone
    with pytest.raises(AssertionError):
        check_result('wrong', ref, out, lse, dqkv, 0.9 * dbias, dls, 0.9 * scr, part, record=False)
    if bpw > 1:
        b, nw = dims[0], (dims[1] // dims[4]) * (dims[2] // dims[4])
        last = emulate_device(qkv[-dims[1] * dims[2]:], dout[-dims[1] * dims[2]:], 1, *dims[1:], ls, bias, mask)
        scr2, part2 = scr.clone(), part.clone()
        scr2[-nw:] -= last[5]
        part2[-nw:] -= last[6]
        with pytest.raises(AssertionError):
            check_result('wrong', ref, out, lse, dqkv, dbias - last[3], dls, scr2, part, record=False)
        with pytest.raises(AssertionError):
            check_result('wrong', ref, out, lse, dqkv, dbias, dls - last[4], scr, part2, record=False)


def test_forward_emulation_at_the_clamped_scale():
    """out and lse at scale 100 (the forward bounds carry expm1(2 Delta) and stay valid there): N = 16, 49, 64"""
    for ws in (4, 7, 8):
        dims = (2, ws, 2 * ws, 2, ws, 0)
        qkv, dout, ls, bias, mask = make_inputs(*dims, seed=ws, ls0=5.0)
        ref = WinRef(qkv, dout, *dims, ls, bias, mask)
        out, lse, *_ = emulate_device(qkv, dout, *dims, ls, bias, mask)
        assert assert_bounded(out, ref.out, ref.m_out, 0.5 * 2.0 ** -8, 0.5, 'out') <= 1
        # lse at 0.7, not 0.5: Delta is the exact worst case of two bf16 roundings per product (2 x 2^-9), with no factor in hand,
        # and at scale 100 a row is dominated by one key, whose 32 product errors hardly average out (measured: 0.54 - 0.64)
        assert assert_bounded(lse, ref.lse, ref.delta + 2.0 ** -18 * (1 + ref.lse.abs()), 0.0, 0.7, 'lse') <= 1
