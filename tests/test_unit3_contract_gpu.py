"""The statistics and backward-prepare entries of the fused residual unit (csrc/unit3.hip: tok_bn_gram_finalize, tok_bn3_bwd_prepare,
tok_bn3_bwd_prepare_ws_floats) element by element against fp64 of exactly the operands each call receives; references, bounds with
their derivations, input makers and case lists are in tests/unit3_clip_ref.py (tests/test_unit3_clip_ref.py holds them to fp64
autograd of the unit).  No element is excluded from a comparison.  (tok_relu_mask_reduce of the same file is covered in
tests/test_conv_contract_gpu.py.)

Every input sits behind NaN guards, every output in a sentinel-filled guarded buffer that holds a prior value under accumulate; after
each call the guards are intact and every owned element is written (an output the call was told to leave out keeps its sentinels).
Every call runs twice and the two runs must be bit-identical, guards included.  The workspace has exactly
tok_bn3_bwd_prepare_ws_floats(p, k) floats behind a guard.

Shapes: the block paths (p in {64, 128, 256}) and the generic paths (tiled fp32 product, split reduction), among them (72, 1032),
whose split reduction has three trailing slices without an element, p = 9 (a ragged 64 x 64 tile on both axes) and p = 2048 (the
largest admitted: 128 KB of LDS in the rows kernel); the partial rows at every count at which fold_partial changes form or starts a
second pass.

Decided here:
  1. tok_bn3_bwd_prepare stores wa in 16-byte segments from a base that was never checked: a misaligned wa is refused with
     TOK_ERR_INVALID now, and include/tok.h says so (test_prepare_refusals).
  2. The generic statistics path takes var = E[y^2] - mean^2 from the fp32 product T.  On the large-mean input (mean 2, std 0.05,
     200 000 rows) no bound small against the value can be derived for it, so its rstd is held, element by element, to 4 x the largest
     deviation of the same formula in the kernel's operation order on a CPU (unit3_clip_ref.large_mean_rstd: about 1e-3 and 2e-3 of
     the value at p = 72 and p = 320), and to the 5e-2 norm ratio against the rows' own variance that the block path is held to.
     Measured on an MI355X: worst |rstd - fp64 of the operands| / rstd 2.7e-4 at p = 72 and 5.1e-4 at p = 320 (block path: 4.9e-8 and
     4.7e-8), norm ratio to the rstd of the rows themselves 5.6e-3 and 2.1e-4 (block: 8.7e-5, 8.2e-5).  The generic path passes
     where the block path passes, with three to four digits less than it, and is left as it is.  Mean 8 was not measured.
  3. count = 1 on a true single row has variance 0, so nothing shows whether the unbiased factor is 1 there;
     test_gram_finalize_one_count_with_variance passes count = 1 with a Z that is not the outer product of zsum.
test_unit3_chain runs the real producers and consumers around the two entries (tok_conv_wgrad, tok_relu_mask_reduce, tok_conv_dgrad,
tok_conv_dgrad_bias) and compares d(input), dW, dgamma and dbeta with the fp64 BatchNorm backward of the unit.
The worst |err| / bound of every tensor is in profiles/unit3_clip_contract_parity_distances.json; the one-line kernel defects this
module and tests/test_grad_clip_contract_gpu.py were run against, with the timings, are in
profiles/unit3_clip_contract_mutation_check.txt."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import BF, ERR_INVALID, F32, U8, _INT_OF, conv_desc, gin, gout, last_error, pack_bits, record_distance
import unit3_clip_ref as M
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
TAG = 'unit3_clip_contract/'
I64 = torch.int64
NBT0 = 7


@pytest.fixture(autouse=True, scope='module')
def _parity_record():
    yield
    M.flush_record()


def ok(rc, what):
    _C.check(rc, what)
    torch.cuda.synchronize()


def written(span, what):
    span.check(what)
    assert int((span.view.view(_INT_OF[span.dtype]) == span.bits).sum()) == 0, f'{what}: owned elements never written'


def intact(span, what):
    span.check(what)
    assert span.untouched(), f'{what}: written although the call was told to leave it'


def twice(run):
    first = [o.buf.view(_INT_OF[o.dtype]).clone() for o in run().values()]
    second = run()
    for a, o in zip(first, second.values()):
        assert torch.equal(a, o.buf.view(_INT_OF[o.dtype])), 'two runs of the same call differ'
    return second


def ins(d, names):
    return {n: gin(d[n].cuda(), 256) for n in names}


def kept(g):
    for n, s in g.items():
        s.check(f'input {n}')


# ---- tok_bn_gram_finalize -----------------------------------------------------------------------------------------------------------
def run_gram(d, eps, running=True, nbt=True, momentum=M.MOMENTUM):
    lib, st = _C.lib(), stream_ptr()
    p, k = d['p'], d['k']
    g = ins(d, ('Z', 'zsum', 'w', 'gamma', 'beta'))

    def run():
        o = {n: gout(k, F32, 256) for n in ('mean', 'rstd', 'scale', 'shift')}
        o['wz'] = gout(k * p, F32, 4 * p + 256)
        o['rm'], o['rv'] = gout(k, F32, 256, init=d['rm'].cuda()), gout(k, F32, 256, init=d['rv'].cuda())
        o['nbt'] = gout(1, I64, 32, init=torch.tensor([NBT0]).cuda())
        ok(lib.tok_bn_gram_finalize(g['Z'].ptr, g['zsum'].ptr, g['w'].ptr, d['count'], p, k, g['gamma'].ptr, g['beta'].ptr,
                                    o['rm'].ptr if running else None, o['rv'].ptr if running else None,
                                    o['nbt'].ptr if nbt else None, momentum, eps, o['mean'].ptr, o['rstd'].ptr, o['scale'].ptr,
                                    o['shift'].ptr, o['wz'].ptr, st), 'bn_gram_finalize')
        for n, s in o.items():
            written(s, n)
        return o
    o = twice(run)
    kept(g)
    return {n: s.value() for n, s in o.items()}


def check_gram(tag, d, v, eps, running=True, nbt=True):
    r = M.gram_finalize_ref(d, eps=eps)
    for n in ('mean', 'rstd', 'scale', 'shift', 'wz') + (('rm', 'rv') if running else ()):
        M.check(tag, n, v[n].reshape(r[n].ref.shape), *r[n])
    if not running:
        assert torch.equal(v['rm'], d['rm']) and torch.equal(v['rv'], d['rv'])
    assert int(v['nbt']) == NBT0 + int(nbt)
    # the all-zero filter row: mean 0, var 0, rstd = (float)(1 / sqrt((double) eps)) exactly, on both paths
    assert float(v['mean'][1]) == 0.0
    assert float(v['rstd'][1]) == float(np.float32(1.0 / np.sqrt(np.float64(np.float32(eps)))))
    assert float(v['scale'][0]) == 0.0 and float(v['shift'][0]) == float(d['beta'][0])        # gamma = 0
    return r


@pytest.mark.parametrize('count', M.COUNTS)
@pytest.mark.parametrize('p,k', M.GRAM_CASES)
def test_gram_finalize(p, k, count):
    eps = M.count_eps(p, count)
    d = M.make_gram(p, k, count)
    tag = TAG + ('gram_finalize block' if M.is_block(p) else 'gram_finalize generic')
    check_gram(tag, d, run_gram(d, eps), eps)


@pytest.mark.parametrize('p,k', [(64, 8), (128, 24), (72, 40), (1024, 16)])
def test_gram_finalize_without_running_statistics(p, k):
    """running statistics NULL (nbt still counted), nbt NULL, both NULL: the same statistics bit for bit, the buffers left out untouched"""
    d = M.make_gram(p, k, 5000)
    full = run_gram(d, M.EPS)
    for running, nbt in ((False, True), (True, False), (False, False)):
        v = run_gram(d, M.EPS, running, nbt)
        check_gram(TAG + 'gram_finalize no running', d, v, M.EPS, running, nbt)
        for n in ('mean', 'rstd', 'scale', 'shift', 'wz') + (('rm', 'rv') if running else ()):
            assert torch.equal(v[n].view(torch.int32), full[n].view(torch.int32)), n


@pytest.mark.parametrize('p', M.LARGE_P)
def test_gram_finalize_large_mean(p):
    """|mean| >> std, 200 000 rows, Z accumulated in fp32: rstd within the bound of its path against fp64 of the operands, element by
    element (block: derived, fp64 ulps; generic: 4 x the largest deviation of the same formula in the kernel's order on the CPU,
    unit3_clip_ref.large_mean_rstd, about 2e-3 of the value), and
    (as tests/test_kernels_gpu.py asks of the block path) within 5e-2 of the variance of the rows themselves by norm ratio and nowhere
    near 1 / sqrt(eps).  Measured here for the first time on the generic path: the figures go to the parity record."""
    d = M.make_large_mean(p)
    v = run_gram(d, M.EPS)
    r = M.gram_finalize_ref(d)
    path = 'block' if M.is_block(p) else 'generic'
    worst_rel = float(((v['rstd'].double() - r['rstd'].ref).abs() / r['rstd'].ref).max())
    want = 1.0 / torch.sqrt(d['var_true'] + M.EPS)
    ratio = float((v['rstd'].double() - want).norm() / want.norm())
    print(f'large mean p={p} ({path}): worst |rstd - fp64 of the operands| / rstd {worst_rel:.3e}, norm ratio to the true rstd {ratio:.3e}')
    w = M.check(None, 'rstd', v['rstd'], *M.large_mean_rstd(d))
    record_distance(TAG + f'gram_finalize large mean {path} p{p}', 'rstd', err_over_bound=w, worst_rel_to_operand_fp64=worst_rel,
                    norm_ratio_to_true=ratio)
    M.check(TAG + f'gram_finalize large mean {path}', 'mean', v['mean'], *r['mean'])
    M.check(TAG + f'gram_finalize large mean {path}', 'wz', v['wz'].reshape(d['k'], p), *r['wz'])
    assert ratio < 5e-2
    assert float(v['rstd'].max()) < 0.5 / (M.EPS ** 0.5)


@pytest.mark.parametrize('p,k', M.ONE_COUNT_CASES)
def test_gram_finalize_one_count_with_variance(p, k):
    """count = 1 on operands of non-zero variance (no single row has them), eps = 1e-5: the running variance takes the factor 1"""
    d = M.make_gram_one_count(p, k)
    check_gram(TAG + 'gram_finalize count 1 with variance', d, run_gram(d, M.EPS), M.EPS)


def test_gram_finalize_refusals():
    lib, st = _C.lib(), stream_ptr()
    d = M.make_gram(64, 8, 5000)
    p, k = 64, 8
    g = ins(d, ('Z', 'zsum', 'w', 'gamma', 'beta'))
    o = {n: gout(k, F32, 256) for n in ('mean', 'rstd', 'scale', 'shift', 'rm', 'rv')}
    o['wz'], o['nbt'] = gout(k * p, F32, 256), gout(1, I64, 32)
    base = [g['Z'].ptr, g['zsum'].ptr, g['w'].ptr, 5000, p, k, g['gamma'].ptr, g['beta'].ptr, o['rm'].ptr, o['rv'].ptr, o['nbt'].ptr,
            0.1, M.EPS, o['mean'].ptr, o['rstd'].ptr, o['scale'].ptr, o['shift'].ptr, o['wz'].ptr]
    bad = [(i, None) for i in (0, 1, 2, 6, 7, 13, 14, 15, 16, 17)] + [(3, 0), (3, -1), (4, 0), (5, 0), (4, -64), (5, -8), (8, None), (9, None)]
    for i, val in bad:
        a = list(base)
        a[i] = val
        rc = lib.tok_bn_gram_finalize(*a, st)
        torch.cuda.synchronize()
        assert rc == ERR_INVALID and 'tok_bn_gram_finalize' in last_error(), (i, val, rc)
    for n, s in o.items():
        intact(s, n)
    kept(g)


# ---- tok_bn3_bwd_prepare ------------------------------------------------------------------------------------------------------------
IN_PREP = ('G', 'w', 'wz', 'zsum', 'partial', 'gamma', 'mean', 'rstd')


def prep_outs(d, pacc, dacc):
    p, k = d['p'], d['k']
    pr = d['prior']
    o = {'dgamma': gout(k, F32, 256, init=pr['dgamma'].cuda() if pacc else None),
         'dbeta': gout(k, F32, 256, init=pr['dbeta'].cuda() if pacc else None),
         'coef': gout(3 * k, F32, 256), 'dw': gout(k * p, F32, 4 * p + 256, init=pr['dw'].cuda() if dacc else None),
         'wa': gout(p * k, BF, 4 * k + 256), 'wb': gout(p * p, BF, 4 * p + 256), 'cvec': gout(p, F32, 256)}
    return o


def run_prepare(d, pacc=0, dacc=0, params=True):
    lib, st = _C.lib(), stream_ptr()
    p, k = d['p'], d['k']
    n_ws = int(lib.tok_bn3_bwd_prepare_ws_floats(p, k))
    assert n_ws == M.ws_floats(p, k)
    g = ins(d, IN_PREP)

    def run():
        o = prep_outs(d, pacc, dacc)
        ws = gout(n_ws, F32, 1024)
        ok(lib.tok_bn3_bwd_prepare(g['G'].ptr, g['w'].ptr, g['wz'].ptr, g['zsum'].ptr, g['partial'].ptr, d['rows'], d['count'], p, k,
                                   g['gamma'].ptr, g['mean'].ptr, g['rstd'].ptr, o['dgamma'].ptr if params else None,
                                   o['dbeta'].ptr if params else None, pacc, o['coef'].ptr, o['dw'].ptr, dacc, o['wa'].ptr,
                                   o['wb'].ptr, o['cvec'].ptr, ws.ptr, st), 'bn3_bwd_prepare')
        ws.check('ws')
        for n, s in o.items():
            if params or n not in ('dgamma', 'dbeta'):
                written(s, n)
            elif not pacc:
                intact(s, n)
        return o
    o = twice(run)
    kept(g)
    return {n: s.value() for n, s in o.items()}


def check_prepare(tag, d, v, pacc=0, dacc=0, params=True):
    r = M.bn3_prepare_ref(d, pacc, dacc)
    for n in ('coef', 'dw', 'wa', 'wb', 'cvec') + (('dgamma', 'dbeta') if params else ()):
        M.check(tag, n + (' accumulated' if (n == 'dw' and dacc) or (n in ('dgamma', 'dbeta') and pacc) else ''),
                v[n].reshape(r[n].ref.shape), *r[n])
    if not params and pacc:
        assert torch.equal(v['dgamma'], d['prior']['dgamma']) and torch.equal(v['dbeta'], d['prior']['dbeta'])


@pytest.mark.parametrize('pacc,dacc', [(0, 0), (1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize('p,k', [c for c in M.PREP_CASES if c[1] % 8 == 0])
def test_bn3_prepare(p, k, pacc, dacc):
    d = M.make_prepare(p, k, rows=3)
    tag = TAG + ('bn3_prepare block' if M.is_block(p) else 'bn3_prepare generic')
    check_prepare(tag, d, run_prepare(d, pacc, dacc), pacc, dacc)


@pytest.mark.parametrize('rows', M.ROWS_CASES)
@pytest.mark.parametrize('p,k', [(64, 8), (72, 40)])
def test_bn3_prepare_partial_rows(p, k, rows):
    """every count at which fold_partial<4 | 8 | 16> is chosen, fills its unroll exactly, or starts another pass; the rows hold
    distinct values, so a skipped or doubled row moves dbeta (and through it c3, dw, cvec) far outside the bound"""
    d = M.make_prepare(p, k, rows=rows)
    check_prepare(TAG + f'bn3_prepare rows fold{M.fold_form(rows)}', d, run_prepare(d))


@pytest.mark.parametrize('pacc', [0, 1])
@pytest.mark.parametrize('p,k', [(64, 8), (72, 40)])
def test_bn3_prepare_without_parameter_gradients(p, k, pacc):
    """dgamma = dbeta = NULL: everything else bit-identical to the full call, the two buffers untouched"""
    d = M.make_prepare(p, k, rows=3)
    full, v = run_prepare(d, pacc, 0), run_prepare(d, pacc, 0, params=False)
    check_prepare(TAG + 'bn3_prepare no params', d, v, pacc, 0, params=False)
    for n in ('coef', 'dw', 'wa', 'wb', 'cvec'):
        assert torch.equal(v[n].view(_INT_OF[v[n].dtype]), full[n].view(_INT_OF[full[n].dtype])), n


def test_prepare_refusals():
    """every NULL operand, sizes <= 0, p > 2048, k % 8 != 0, a misaligned wa: TOK_ERR_INVALID, a message, nothing written"""
    lib, st = _C.lib(), stream_ptr()
    d = M.make_prepare(64, 8, rows=3)
    p, k = 64, 8
    g = ins(d, IN_PREP)
    o = prep_outs(d, 0, 0)
    ws = gout(M.ws_floats(p, k), F32, 1024)
    base = [g['G'].ptr, g['w'].ptr, g['wz'].ptr, g['zsum'].ptr, g['partial'].ptr, 3, 4000, p, k, g['gamma'].ptr, g['mean'].ptr,
            g['rstd'].ptr, o['dgamma'].ptr, o['dbeta'].ptr, 0, o['coef'].ptr, o['dw'].ptr, 0, o['wa'].ptr, o['wb'].ptr, o['cvec'].ptr,
            ws.ptr]
    bad = [(i, None) for i in (0, 1, 2, 3, 4, 9, 10, 11, 15, 16, 18, 19, 20, 21)]
    bad += [(5, 0), (5, -1), (6, 0), (6, -5), (7, 0), (7, -64), (7, 2049), (8, 0), (8, -8), (8, 12), (8, 4)]
    bad += [(18, o['wa'].ptr + 2), (18, o['wa'].ptr + 8)]
    for i, val in bad:
        a = list(base)
        a[i] = val
        rc = lib.tok_bn3_bwd_prepare(*a, st)
        torch.cuda.synchronize()
        assert rc == ERR_INVALID and 'tok_bn3_bwd_prepare' in last_error(), (i, val, rc)
    for n, s in o.items():
        intact(s, n)
    intact(ws, 'ws')
    kept(g)


# ---- the chain: real producers and consumers of the two entries' operands --------------------------------------------------------------
def _wgrad(D, x, dy, k, c, ws_bytes):
    lib, st = _C.lib(), stream_ptr()
    dw, ws = gout(k * c, F32, 4 * c + 256), gout(max(ws_bytes, 1), U8, 1 << 16)
    ok(lib.tok_conv_wgrad(D, x.ptr, dy.ptr, dw.ptr, k, c, ws.ptr, ws_bytes, 0, st), 'conv_wgrad')
    written(dw, 'dw of tok_conv_wgrad')
    ws.check('ws of tok_conv_wgrad')
    return dw


@pytest.mark.parametrize('m,p,k', M.CHAIN_CASES)
def test_unit3_chain(m, p, k):
    """tok_conv_wgrad on (z, z) and on (dz, z), tok_relu_mask_reduce, tok_bn_gram_finalize, tok_bn3_bwd_prepare, tok_conv_dgrad +
    tok_conv_dgrad_bias, every operand handed on as the producer wrote it (the [2][rows][k] partial rows, Z and G of the
    weight-gradient launch, wa in the data-gradient pack layout): d(input), dW, dgamma and dbeta element by element against the fp64
    BatchNorm backward of the unit (unit3_clip_ref.make_chain has the bounds); the whole chain twice with identical bits"""
    lib, st = _C.lib(), stream_ptr()
    c = M.make_chain(m, p, k)
    n, h = m // 64, 8
    assert n * h * h == m
    dzz, dkz = conv_desc(n, h, h, p, p, 1, 1, 0), conv_desc(n, h, h, p, k, 1, 1, 0)
    Dzz, Dkz = ctypes.byref(dzz), ctypes.byref(dkz)
    rows = int(lib.tok_bn_bwd_rows(m, k))
    n_ws = int(lib.tok_bn3_bwd_prepare_ws_floats(p, k))
    zg, doutg = gin(c['z'].cuda(), 128 * p), gin(c['dout'].cuda(), 128 * k)
    maskg = gin(pack_bits(c['mask']).cuda(), 128 * k // 8)
    small = ins(c, ('w', 'gamma', 'beta', 'zsum'))

    def run():
        Z = _wgrad(Dzz, zg, zg, p, p, int(lib.tok_conv_wgrad_ws_bytes(Dzz)))
        dz, part = gout(m * k, BF, 128 * k), gout(2 * rows * k, F32, 4 * k + 256)
        ok(lib.tok_relu_mask_reduce(doutg.ptr, maskg.ptr, m, k, dz.ptr, part.ptr, st), 'relu_mask_reduce')
        written(dz, 'dz')
        written(part, 'partial rows')
        G = _wgrad(Dkz, zg, dz, k, p, int(lib.tok_conv_wgrad_ws_bytes(Dkz)))
        f = {n_: gout(k, F32, 256) for n_ in ('mean', 'rstd', 'scale', 'shift')}
        f['wz'] = gout(k * p, F32, 4 * p + 256)
        ok(lib.tok_bn_gram_finalize(Z.ptr, small['zsum'].ptr, small['w'].ptr, m, p, k, small['gamma'].ptr, small['beta'].ptr, None, None,
                                    None, 0.1, M.EPS, f['mean'].ptr, f['rstd'].ptr, f['scale'].ptr, f['shift'].ptr, f['wz'].ptr, st),
           'bn_gram_finalize')
        o = {'dgamma': gout(k, F32, 256), 'dbeta': gout(k, F32, 256), 'coef': gout(3 * k, F32, 256), 'dw': gout(k * p, F32, 4 * p + 256),
             'wa': gout(p * k, BF, 4 * k + 256), 'wb': gout(p * p, BF, 4 * p + 256), 'cvec': gout(p, F32, 256)}
        ws = gout(n_ws, F32, 1024)
        ok(lib.tok_bn3_bwd_prepare(G.ptr, small['w'].ptr, f['wz'].ptr, small['zsum'].ptr, part.ptr, rows, m, p, k, small['gamma'].ptr,
                                   f['mean'].ptr, f['rstd'].ptr, o['dgamma'].ptr, o['dbeta'].ptr, 0, o['coef'].ptr, o['dw'].ptr, 0,
                                   o['wa'].ptr, o['wb'].ptr, o['cvec'].ptr, ws.ptr, st), 'bn3_bwd_prepare')
        ws.check('ws')
        o['dx'] = gout(m * p, BF, 128 * p)
        ok(lib.tok_conv_dgrad(Dkz, dz.ptr, o['wa'].ptr, o['dx'].ptr, 0, st), 'conv_dgrad')
        ok(lib.tok_conv_dgrad_bias(Dzz, zg.ptr, o['wb'].ptr, o['cvec'].ptr, o['dx'].ptr, 1, None, None, None, st), 'conv_dgrad_bias')
        o.update(f, Z=Z, G=G, dz=dz)
        for name, sp in o.items():
            written(sp, name)
        return o
    o = twice(run)
    for g in (zg, doutg, maskg):
        g.check('an input of the chain')
    kept(small)
    tag = TAG + f'chain p{p}'
    assert torch.equal(o['dz'].value().view(torch.int16).reshape(m, k), c['dz'].view(torch.int16))      # the masked gradient is exact
    for name in ('dx', 'dw', 'dgamma', 'dbeta'):
        ref = c['out'][name]
        M.check(tag, name, o[name].value().reshape(ref.ref.shape), *ref)
    # the operands the real producers handed on, against fp64 of the same rows: fp32 chains of m products (any split order)
    zd, dzd = c['z'].double(), c['dz'].double()
    M.check(tag, 'Z', o['Z'].value().reshape(p, p), c['Z'], (m + 8) * 2.0 ** -24 * (zd.abs().t() @ zd.abs()))
    M.check(tag, 'G', o['G'].value().reshape(k, p), c['G'], (m + 8) * 2.0 ** -24 * (dzd.abs().t() @ zd.abs()))
