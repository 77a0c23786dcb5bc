"""The HRNet-OCR entries of csrc/ocr.hip (tok_pix_class_matmul, tok_class_pix_expand, tok_weighted_pool, tok_softmax_rows_f32 /
_bwd_f32, tok_softmax_cols_fwd / _bwd, tok_channel_scale) and the DaViT entries of csrc/channel_attn.hip (tok_chan_gram,
tok_chan_apply, tok_scale_rows_add, tok_dwconv3x3, tok_dwconv3x3_wgrad) element by element against fp64 of the same inputs;
references, bounds, input makers and the case lists are in tests/ocr_chan_ref.py (tests/test_ocr_chan_ref.py: every reference is
torch's own operation and autograd in fp64, an fp32 run stays inside half of every bound, wrong variants are rejected).  No element is
excluded from any comparison.

Every input sits behind NaN pads and NaN guards, every output and workspace in a sentinel-filled guarded buffer; after each call the
guards are intact, every owned element is written and finite, and the pad columns hold what include/tok.h says.  Every call runs twice
and the two runs must be bit-identical, pads and guards included (weighted_pool, chan_gram and dwconv3x3_wgrad promise a fixed order).
Every case names the launch class it is meant to hit and asserts it against a restatement of the launcher's rule
(ocr_chan_ref.grid_class / lane_class / pool_class / tile_class / wgrad_geometry), so that a threshold change moves a test instead of
silently moving coverage.  Two images everywhere (except where the issue fixes n of the weight gradient), so the per-image offset matters.

Three suspects are decided here:
  1. tok_channel_scale multiplied the pad columns of x by 0 (NaN in a pad of x -> NaN in the pad of out): fixed to a select;
     test_channel_scale fails on the old library at every case with ld > c ("pad columns c..ld are not zero": the NaN pad of x times 0).
  2. only the pitch was checked for the 16-byte accesses: a base that is not 16-byte aligned is refused now in tok_chan_gram,
     tok_chan_apply, tok_scale_rows_add, tok_class_pix_expand, tok_channel_scale and tok_dwconv3x3 (test_misaligned_operands_are_refused;
     the old library launched such a call; it was not run).
  3. tok_dwconv3x3_wgrad launches fewer blocks than tok_dwconv3x3_wgrad_blocks sizes: correct as it is, the fold uses the launched
     count; test_dwconv3x3_wgrad[25-41-...] pins it and the untouched tail of `partial`.
The worst |err| / bound of every tensor of every kernel family goes to profiles/ocr_chan_contract_parity_distances.json;
profiles/ocr_chan_contract_mutation_check.txt lists the hand-made kernel defects this module was run against.

On an MI355X the module (105 tests) runs in 5.4 s; the slowest case is test_dwconv3x3_second_trip, 0.98 s (8.5 M outputs compared with
fp64 on the host), then the first one, test_pix_class_matmul[1-1-1-...], 0.48 s (it pays the first launch), and the other second-trip
cases: test_scale_rows_add[8200-1024-...] 0.47 s, test_class_pix_expand[4100-1-513-...] 0.41 s, test_channel_scale[4100-513-520-...]
0.33 s; every other case is below 0.04 s."""
import pytest
import torch

from helpers import BF, ERR_INVALID, F32, GuardedSpan, Mat, _INT_OF, cdiv, last_error
import ocr_chan_ref as M
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
TAG = 'ocr_chan_contract/'
B = M.IMAGES
HD = M.HD


@pytest.fixture(autouse=True, scope='module')
def _parity_record():
    """one line per kernel family and tensor: the worst |err| / bound over every case and variant of the family"""
    yield
    M.flush_record()


def mat_in(t, ld=None, off=0):
    """an input, its last axis the columns, pitch ld: NaN in the pads, in front and in both guards"""
    t = t.reshape(-1, t.shape[-1])
    return Mat(t.shape[0], t.shape[1], ld, dtype=t.dtype, init=t.cuda(), nan=True, off=off)


def mat_out(rows, cols, ld=None, dtype=BF, prior=None):
    """an output: sentinels everywhere, the owned elements holding `prior` under accumulate"""
    return Mat(rows, cols, ld, dtype=dtype, init=None if prior is None else prior.reshape(rows, cols).cuda())


def done(m, what, zero_to=None):
    """guards and the elements in front intact, every owned element written and finite; pad columns cols .. zero_to are zero, the
    rest of the pitch holds its sentinels (zero_to None: the whole pad does)"""
    m.span.check(what)
    it = _INT_OF[m.dtype]
    iv = m.full.view(it)
    assert bool((m.span.view[:m.off].view(it) == m.bits).all()), f'{what}: elements in front overwritten'
    assert int((iv[:, :m.cols] == m.bits).sum()) == 0, f'{what}: owned elements never written'
    assert bool(torch.isfinite(m.view.float()).all()), f'{what}: not finite'
    z = m.cols if zero_to is None else zero_to
    assert bool((m.full[:, m.cols:z] == 0).all()), f'{what}: pad columns {m.cols}..{z} are not zero'
    assert bool((iv[:, z:] == m.bits).all()), f'{what}: pad columns from {z} overwritten'


def kept(*ms):
    """inputs: pads, guards and the elements in front still hold their NaN"""
    for m in ms:
        m.done('an input', finite=False)


def bits(*ms):
    """every element of the buffers behind Mats / GuardedSpans, as integers (bit-identity, pads and guards included)"""
    out = []
    for m in ms:
        b = m.span.buf if isinstance(m, Mat) else m.buf
        out.append(b.view({2: torch.int16, 4: torch.int32}[b.element_size()]).clone())
    return out


def twice(run):
    """run() -> the output operands of one fresh call; two calls give the same bits"""
    first = run()
    a = bits(*first)
    second = run()
    for x, y in zip(a, bits(*second)):
        assert torch.equal(x, y), 'two runs of the same call differ'
    return second


def ok(rc, what):
    _C.check(rc, what)
    torch.cuda.synchronize()


def sums_to(what, v, dim, target, out):
    """sum(v, dim) == target within the sum of the elements' bounds, in fp64 of the device values"""
    s = v.double().cpu().sum(dim)
    lim = out.bound().sum(dim)
    assert bool(((s - target).abs() <= lim).all()), f'{what}: sums off by {float(((s - target).abs() - lim).max()):.3e} more than the bounds'


# ---- OCR ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,k,c,ldx,ldm,cls', M.PCM_CASES)
def test_pix_class_matmul(n, k, c, ldx, ldm, cls):
    """(5, 64, 256) is the largest class matrix accepted: exactly 64 KB of LDS"""
    lib, st = _C.lib(), stream_ptr()
    assert M.pcm_class(n, c) == cls
    d = M.make_ocr(B, n, k, c, seed=n + k + c)
    xg, mg = mat_in(d['x'], ldx), mat_in(d['m'], ldm)
    for scale in (1.0, 0.37):
        def run():
            og = mat_out(B * n, k, dtype=F32)
            ok(lib.tok_pix_class_matmul(xg.ptr, ldx, mg.ptr, ldm, B, n, k, c, scale, og.ptr, st), 'pix_class_matmul')
            done(og, 'out')
            return [og]
        og, = twice(run)
        M.check(TAG + 'pix_class_matmul', 'out', og.view.reshape(B, n, k), M.pix_class_matmul_ref(d['x'], d['m'], scale))
    kept(xg, mg)


@pytest.mark.parametrize('n,k,c,ldm,ldo,cls', M.CPE_CASES)
def test_class_pix_expand(n, k, c, ldm, ldo, cls):
    """columns c .. round8(c) are 0 when fresh and re-stored as read under accumulate, the rest of the pitch is never touched;
    (3, 64, 250) is the largest class matrix accepted (64 x 256 floats)"""
    lib, st = _C.lib(), stream_ptr()
    assert M.grid_class(n * cdiv(c, 8), 1024) == cls
    d = M.make_ocr(B, n, k, c, seed=n + k + c)
    wg, mg = mat_in(d['w']), mat_in(d['m'], ldm)
    for scale in ((1.0, 0.37) if n < 1000 else (0.37,)):
        for prior in (None, d['prior_nc']):
            def run():
                og = mat_out(B * n, c, ldo, prior=prior)
                ok(lib.tok_class_pix_expand(wg.ptr, mg.ptr, ldm, B, n, k, c, scale, og.ptr, ldo, int(prior is not None), st), 'class_pix_expand')
                done(og, 'out', zero_to=None if prior is not None else cdiv(c, 8) * 8)
                return [og]
            og, = twice(run)
            M.check(TAG + 'class_pix_expand', 'out' if prior is None else 'out accumulated', og.view.reshape(B, n, c),
                    M.class_pix_expand_ref(d['w'], d['m'], scale, prior))
    kept(wg, mg)


@pytest.mark.parametrize('case,cls', list(zip(M.WP_CASES, M.WP_CLASSES)))
def test_weighted_pool(case, cls):
    """`partial` holds exactly images * chunks * k * c floats; a class of zero weights pools to exactly 0; fixed order"""
    lib, st = _C.lib(), stream_ptr()
    n, k, c, ldx, ldo = case
    assert M.pool_class(n, k, c) == cls
    chunks = lib.tok_weighted_pool_chunks(n)
    assert chunks == cdiv(n, 512)
    d = M.make_ocr(B, n, k, c, seed=n + k + c)
    wg, xg = mat_in(d['w']), mat_in(d['x'], ldx)
    for prior in (None, d['prior_kc']):
        def run():
            og, part = mat_out(B * k, c, ldo, prior=prior), GuardedSpan(B * chunks * k * c, F32, 64)
            ok(lib.tok_weighted_pool(wg.ptr, xg.ptr, ldx, B, n, k, c, 0.25, part.ptr, og.ptr, ldo, int(prior is not None), st), 'weighted_pool')
            done(og, 'out')
            part.check('partial')
            assert int((part.view.view(torch.int32) == part.bits).sum()) == 0, 'partial: elements never written'
            return [og, part]
        og, _ = twice(run)
        M.check(TAG + 'weighted_pool', 'out' if prior is None else 'out accumulated', og.view.reshape(B, k, c), M.weighted_pool_ref(d['w'], d['x'], 0.25, prior))
        if k > 1 and prior is None:
            assert bool((og.view.reshape(B, k, c)[:, k - 1] == 0).all())
    kept(wg, xg)


def rows_class(rows):
    return M.grid_class(rows, 2048)


@pytest.mark.parametrize('rows,k', M.SR_CASES)
def test_softmax_rows(rows, k):
    """no 64-class limit; row 0 one +80 among -80s, row 1 constant, row 2 of -0.0; the backward takes the p the forward stored"""
    lib, st = _C.lib(), stream_ptr()
    assert rows_class(rows) == ('below one block' if rows < 256 else 'second trip' if rows > 2048 * 256 else 'blocks')
    x, dp = M.make_softmax_rows(rows, k, seed=rows + k)
    xg, dg = mat_in(x), mat_in(dp)
    pg = mat_out(rows, k, dtype=F32)
    ok(lib.tok_softmax_rows_f32(xg.ptr, rows, k, pg.ptr, st), 'softmax_rows')
    done(pg, 'p')
    ref = M.softmax_rows_ref(x)
    M.check(TAG + 'softmax_rows', 'p', pg.view, ref)
    sums_to('rows of p', pg.view, 1, 1.0, ref)
    if rows > 1:
        assert bool((pg.view[1] == pg.view[1, 0]).all()), 'a constant row'
    if k > 1:
        assert float(pg.view[0, k // 2]) == 1.0 and float(pg.view[0].sum()) == 1.0, 'one +80 among -80s'
    p = pg.value()
    p_in = mat_in(p)

    def run():
        og = mat_out(rows, k, dtype=F32)
        ok(lib.tok_softmax_rows_bwd_f32(p_in.ptr, dg.ptr, rows, k, og.ptr, st), 'softmax_rows_bwd')
        done(og, 'dx')
        return [og]
    og, = twice(run)
    M.check(TAG + 'softmax_rows', 'dx', og.view, M.softmax_rows_bwd_ref(p, dp))
    kept(xg, dg, p_in)


@pytest.mark.parametrize('n,k,ld', M.SC_CASES)
def test_softmax_cols(n, k, ld):
    """scale 1 and 0.37; every column of p sums to 1; the backward writes the whole pitch: 0 past k when fresh, unchanged under accumulate"""
    lib, st = _C.lib(), stream_ptr()
    assert M.tile_class(n, 256) == {1: '1 x 256, ragged', 255: '1 x 256, ragged', 256: '1 x 256, full', 257: '2 x 256, ragged', 1000: '4 x 256, ragged'}[n]
    l, dp, prior = M.make_softmax_cols(B, n, k, seed=n + k)
    lg, dg = mat_in(l, ld), mat_in(dp)
    for scale in M.SC_SCALES:
        pg = mat_out(B * n, k, dtype=F32)
        ok(lib.tok_softmax_cols_fwd(lg.ptr, ld, B, n, k, scale, pg.ptr, st), 'softmax_cols_fwd')
        done(pg, 'p')
        ref = M.softmax_cols_fwd_ref(l, scale)
        M.check(TAG + 'softmax_cols', 'p', pg.view.reshape(B, n, k), ref)
        sums_to('columns of p', pg.view.reshape(B, n, k), 1, 1.0, ref)
        p = pg.value().reshape(B, n, k)
        p_in = mat_in(p)
        for pr in (None, prior):
            def run():
                og = mat_out(B * n, k, ld, prior=pr)
                ok(lib.tok_softmax_cols_bwd(p_in.ptr, dg.ptr, B, n, k, scale, og.ptr, ld, int(pr is not None), st), 'softmax_cols_bwd')
                done(og, 'dlogits', zero_to=None if pr is not None else ld)
                return [og]
            og, = twice(run)
            M.check(TAG + 'softmax_cols', 'dlogits' if pr is None else 'dlogits accumulated', og.view.reshape(B, n, k), M.softmax_cols_bwd_ref(p, dp, scale, pr))
        kept(p_in)
    kept(lg, dg)


@pytest.mark.parametrize('n,c,ld,cls', M.CS_CASES)
def test_channel_scale(n, c, ld, cls):
    """Suspect 1.  The kernel computed x * 0 on the pad columns c .. ld, so the NaN pads of x here became NaN in the pads of out: on the
    old library this test fails at every case with ld > c on "pad columns c..ld are not zero" (fresh) and "pad columns overwritten"
    (accumulate: sentinel + NaN).  Now a select: the pad of out is 0 when fresh and unchanged under accumulate (include/tok.h).  The
    gate holds an exact 0 and 1 / 0.7."""
    lib, st = _C.lib(), stream_ptr()
    assert M.grid_class(n * (ld // 8), 1024) == cls
    x, s, prior = M.make_channel_scale(B, n, c, seed=n + c)
    xg, sg = mat_in(x, ld), mat_in(s)
    for pr in (None, prior):
        def run():
            og = mat_out(B * n, c, ld, prior=pr)
            ok(lib.tok_channel_scale(xg.ptr, sg.ptr, og.ptr, int(pr is not None), B, n, c, ld, st), 'channel_scale')
            done(og, 'out', zero_to=None if pr is not None else ld)
            return [og]
        og, = twice(run)
        M.check(TAG + 'channel_scale', 'out' if pr is None else 'out accumulated', og.view.reshape(B, n, c), M.channel_scale_ref(x, s, pr))
        if pr is None:
            assert bool((og.view.reshape(B, n, c)[0, :, 0] == 0).all()), 'a gate of exactly 0'
    kept(xg, sg)


# ---- DaViT -------------------------------------------------------------------------------------------------------------------------
def qkv_mat(q, k, v):
    """[b * rpi][3c] with a NaN pad of 8 columns; returns (Mat, ld, byte offsets of the three thirds)"""
    c = q.shape[-1]
    m = mat_in(torch.cat([q, k, v], -1), 3 * c + 8)
    return m, 3 * c + 8, (0, 2 * c, 4 * c)


@pytest.mark.parametrize('heads', M.HEADS)
@pytest.mark.parametrize('rpi', M.CG_RPI)
def test_chan_gram(rpi, heads):
    """tokens in tiles of 64: 1, 63, 64, 65, 200; x in a matrix of its own (ldx = c + 8), y the v third of a qkv matrix (ldy = 3c + 8);
    a planted logit above 50; rows of mode 1 sum to 1, rows of mode 2 (of the A that mode 1 stored) to 0"""
    lib, st = _C.lib(), stream_ptr()
    assert M.tile_class(rpi, 64) == {1: '1 x 64, ragged', 63: '1 x 64, ragged', 64: '1 x 64, full', 65: '2 x 64, ragged', 200: '4 x 64, ragged'}[rpi]
    c, u = heads * HD, B * heads
    scale = HD ** -0.5
    x, y, _, dout = M.make_chan(B, rpi, heads, seed=rpi + heads)
    xg, dg = mat_in(x, c + 8), mat_in(dout, c + 8)
    qg, ld, offs = qkv_mat(dout, x, y)
    outs = {}
    for mode in (0, 1):
        def run():
            og = mat_out(u * HD, HD, dtype=F32)
            ok(lib.tok_chan_gram(xg.ptr, c + 8, qg.ptr + offs[2], ld, rpi, B, heads, scale, mode, None, og.ptr, st), 'chan_gram')
            done(og, 'out')
            return [og]
        og, = twice(run)
        ref = M.chan_gram_ref(x, y, scale, mode)
        M.check(TAG + 'chan_gram', ('G', 'A')[mode], og.view.reshape(u, HD, HD), ref)
        outs[mode] = og
    assert float(outs[0].view[0, 0]) > 50
    sums_to('rows of A', outs[1].view.reshape(u, HD, HD), 2, 1.0, ref)
    a = outs[1].value().reshape(u, HD, HD)
    a_in = mat_in(a)

    def run2():
        og = mat_out(u * HD, HD, dtype=F32)
        ok(lib.tok_chan_gram(dg.ptr, c + 8, qg.ptr + offs[1], ld, rpi, B, heads, 1.0, 2, a_in.ptr, og.ptr, st), 'chan_gram')
        done(og, 'out')
        return [og]
    og, = twice(run2)
    ref = M.chan_gram_ref(dout, x, 1.0, 2, a)
    M.check(TAG + 'chan_gram', 'dS', og.view.reshape(u, HD, HD), ref)
    # sum_j A_j (G_j - sum A G) = (1 - sum A) sum A G: 0 up to the distance of the stored rows of A from 1
    sums_to('rows of dS', og.view.reshape(u, HD, HD), 2, ref.ref.sum(2), ref)
    g = M.chan_gram(dout, x, 1.0, 0)
    assert bool((ref.ref.sum(2).abs() <= (a.double().sum(2) - 1).abs() * (g * a.double()).sum(2).abs() + 1e-12 * (g * a.double()).abs().sum(2)).all())
    kept(xg, dg, qg, a_in)


@pytest.mark.parametrize('heads', M.HEADS)
@pytest.mark.parametrize('rpi', M.CA_RPI)
def test_chan_apply(rpi, heads):
    """tokens in tiles of 128; x the q third of a qkv matrix, out the MIDDLE third of a wider gradient matrix (as the engine writes dk):
    nothing outside its heads * 32 columns is touched; both `transposed` settings are adjoint to each other"""
    lib, st = _C.lib(), stream_ptr()
    assert M.tile_class(rpi, 128) == {1: '1 x 128, ragged', 127: '1 x 128, ragged', 128: '1 x 128, full', 129: '2 x 128, ragged', 300: '3 x 128, ragged'}[rpi]
    c = heads * HD
    x, y, m, _ = M.make_chan(B, rpi, heads, seed=rpi + heads)
    qg, ld, offs = qkv_mat(x, y, y)
    mg = mat_in(m)
    it = torch.int16

    def apply(src_off, transposed, scale):
        def run():
            wide = Mat(B * rpi, 3 * c, ld)
            ok(lib.tok_chan_apply(qg.ptr + src_off, ld, mg.ptr, transposed, scale, rpi, B, heads, wide.ptr + 2 * c, ld, st), 'chan_apply')
            wide.span.check('out')
            iv = wide.full.view(it)
            assert bool((iv[:, :c] == wide.bits).all()) and bool((iv[:, 2 * c:] == wide.bits).all()), 'columns outside the third written'
            mid = wide.full[:, c:2 * c]
            assert int((mid.view(it) == wide.bits).sum()) == 0 and bool(torch.isfinite(mid.float()).all()), 'owned elements'
            return [wide]
        wide, = twice(run)
        return wide.full[:, c:2 * c].reshape(B, rpi, c).cpu()
    for scale in (1.0, HD ** -0.5):
        o = {}
        for transposed in (0, 1):
            src = (x, y)[transposed]
            o[transposed] = apply(offs[transposed], transposed, scale)
            ref = M.chan_apply_ref(src, m, transposed, scale)
            M.check(TAG + 'chan_apply', 'out' if not transposed else 'out transposed', o[transposed], ref)
            o[transposed, 'bound'] = ref.bound()
        lhs, rhs = (o[0].double() * y.double()).sum(), (x.double() * o[1].double()).sum()
        lim = (o[0, 'bound'] * y.double().abs()).sum() + (x.double().abs() * o[1, 'bound']).sum()
        assert abs(float(lhs - rhs)) <= float(lim), f'<Mx, y> = {float(lhs)!r}, <x, M^T y> = {float(rhs)!r}'
    kept(qg, mg)


@pytest.mark.parametrize('rows,ld,rps,with_a,acc', M.SRA_CASES)
def test_scale_rows_add(rows, ld, rps, with_a, acc):
    """a and row_scale NULL or not, rps dividing rows (64 / 16) and not (50 / 16), a row_scale of 0 and of 1 / 0.7; 8200 x 1024 is past
    the 4096 blocks.  With row_scale NULL there is no product to contract: the result is bf16 of the fp32 formula bit for bit."""
    lib, st = _C.lib(), stream_ptr()
    assert M.grid_class(rows * (ld // 8), 4096) == ('second trip' if rows == 8200 else 'below one block' if rows * ld < 2048 else 'blocks')
    a, b, rs, prior = M.make_rows_add(rows, ld, rps, seed=rows + ld)
    a, prior = (a if with_a else None), (prior if acc else None)
    ag, bg, rg = None if a is None else mat_in(a), mat_in(b), None if rs is None else mat_in(rs)

    def run():
        og = mat_out(rows, ld, prior=prior)
        ok(lib.tok_scale_rows_add(None if a is None else ag.ptr, bg.ptr, None if rs is None else rg.ptr, rps, og.ptr, acc, rows, ld, st), 'scale_rows_add')
        done(og, 'out')
        return [og]
    og, = twice(run)
    M.check(TAG + 'scale_rows_add', 'out', og.view, M.scale_rows_add_ref(a, b, rs, rps, prior))
    if rs is None:
        want = b.float()
        want = want + a.float() if a is not None else want
        want = want + prior.float() if prior is not None else want
        assert torch.equal(og.value(), want.to(BF)), 'bf16 of the fp32 formula, bit for bit'
    else:
        want = torch.zeros(rps, ld)                      # sample 0 has row_scale 0: 0 * b + a is a, whether or not it is one fma
        want = want + a[:rps].float() if a is not None else want
        want = want + prior[:rps].float() if prior is not None else want
        assert torch.equal(og.value()[:rps].float(), want.to(BF).float()), 'a row_scale of exactly 0 drops b'
    kept(*[m for m in (ag, bg, rg) if m is not None])


def _dwconv(n, h, w, c, ld, variants, seed):
    lib, st = _C.lib(), stream_ptr()
    d = M.make_dwconv(n, h, w, c, seed=seed)
    xg, gg, wg, bg = mat_in(d['x'], ld), mat_in(d['dout'], ld), mat_in(d['wt']), mat_in(d['bias'])
    res = {}
    for with_bias, flip, acc in variants:
        src, srcg = (d['dout'], gg) if flip else (d['x'], xg)
        bias, prior = (d['bias'] if with_bias else None), (d['prior'] if acc else None)

        def run():
            og = mat_out(n * h * w, c, ld, prior=prior)
            ok(lib.tok_dwconv3x3(srcg.ptr, wg.ptr, bg.ptr if with_bias else None, og.ptr, acc, flip, n, h, w, c, ld, st), 'dwconv3x3')
            done(og, 'out', zero_to=None if acc else ld)
            return [og]
        og, = twice(run)
        ref = M.dwconv3x3_ref(src, d['wt'], bias, flip, prior)
        M.check(TAG + 'dwconv3x3', ('out', 'dx')[flip] + (' accumulated' if acc else ''), og.view.reshape(n, h, w, c), ref)
        res[with_bias, flip, acc] = (og.value().reshape(n, h, w, c).double(), ref.bound())
    kept(xg, gg, wg, bg)
    return d, res


@pytest.mark.parametrize('c,ld', M.DW_COLS)
@pytest.mark.parametrize('h,w', M.DW_MAPS)
def test_dwconv3x3(h, w, c, ld):
    """bias NULL or not, flip, accumulate; c = 264: the clamped filter loads of the last channel group; flip = 1 is the adjoint of flip = 0"""
    assert M.grid_class(B * h * w * (ld // 8), 4096) in ('below one block', 'blocks')
    d, res = _dwconv(B, h, w, c, ld, [(b_, f_, a_) for b_ in (0, 1) for f_ in (0, 1) for a_ in (0, 1)], seed=h + w + c)
    (y, by), (dx, bx) = res[0, 0, 0], res[0, 1, 0]
    x, g = d['x'].double(), d['dout'].double()
    lhs, rhs = (y * g).sum(), (x * dx).sum()
    lim = (by * g.abs()).sum() + (x.abs() * bx).sum()
    assert abs(float(lhs - rhs)) <= float(lim), f'<conv(x), g> = {float(lhs)!r}, <x, conv_flip(g)> = {float(rhs)!r}'


def test_dwconv3x3_second_trip():
    n, h, w, c, ld = M.DW_BIG
    assert M.grid_class(n * h * w * (ld // 8), 4096) == 'second trip'
    _dwconv(n, h, w, c, ld, [(1, 0, 0)], seed=11)


@pytest.mark.parametrize('n,h,w,c,ld,geo', M.DWG_CASES)
def test_dwconv3x3_wgrad(n, h, w, c, ld, geo):
    """Suspect 3, pinned as correct: at 1025 rows the call launches 513 blocks of two rows while tok_dwconv3x3_wgrad_blocks sizes
    `partial` for 1024; the fold runs over the launched count, and the tail of `partial` keeps its sentinels.  dw only, db only, both;
    c = 264: the channel loop's second trip; fixed order."""
    lib, st = _C.lib(), stream_ptr()
    sized, rpb, launched = M.wgrad_geometry(n, h)
    assert (sized, rpb, launched) == geo and lib.tok_dwconv3x3_wgrad_blocks(n, h) == sized
    d = M.make_dwconv(n, h, w, c, seed=n + h)
    xg, gg = mat_in(d['x'], ld), mat_in(d['dout'], ld)
    for want_w, want_b in ((1, 1), (1, 0), (0, 1)):
        for acc in (0, 1):
            pw, pb = (d['prior_dw'], d['prior_db']) if acc else (None, None)

            def run():
                wg, bg = mat_out(c, 9, dtype=F32, prior=pw), mat_out(1, c, dtype=F32, prior=pb)
                part = GuardedSpan(sized * c * 10, F32, 64)
                ok(lib.tok_dwconv3x3_wgrad(xg.ptr, gg.ptr, n, h, w, c, ld, part.ptr, wg.ptr if want_w else None, bg.ptr if want_b else None,
                                           acc, st), 'dwconv3x3_wgrad')
                part.check('partial')
                pv = part.view.view(torch.int32)
                assert int((pv[:launched * c * 10] == part.bits).sum()) == 0, 'partial: rows of launched blocks never written'
                assert bool((pv[launched * c * 10:] == part.bits).all()), 'partial: the tail past the launched blocks was written'
                for m_, wanted, what in ((wg, want_w, 'dw'), (bg, want_b, 'db')):
                    if wanted:
                        done(m_, what)
                    elif not acc:
                        m_.intact(what)
                return [wg, bg, part]
            wg, bg, _ = twice(run)
            ref = M.dwconv3x3_wgrad_ref(d['x'], d['dout'], pw, pb)
            if want_w:
                M.check(TAG + 'dwconv3x3_wgrad', 'dw' + (' accumulated' if acc else ''), wg.view, ref['dw'])
            if want_b:
                M.check(TAG + 'dwconv3x3_wgrad', 'db' + (' accumulated' if acc else ''), bg.view[0], ref['db'])
    kept(xg, gg)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def refused(rc, entry, *outs):
    assert rc == ERR_INVALID, (entry, rc)
    assert entry in last_error(), (entry, last_error())
    torch.cuda.synchronize()
    for o in outs:
        if isinstance(o, Mat):
            o.intact(entry)
        else:
            o.check(entry)
            assert o.untouched(), f'{entry}: workspace written by a refused call'


def test_refusals():
    """every refused call returns TOK_ERR_INVALID, names its entry in tok_last_error() and leaves every output untouched"""
    lib, st = _C.lib(), stream_ptr()
    n, k, c = 5, 3, 16
    d = M.make_ocr(B, n, 64, 264, seed=1)
    xg, mg, wg = mat_in(d['x']), mat_in(d['m']), mat_in(d['w'])
    o32, obf, part = mat_out(B * n, 65, dtype=F32), mat_out(B * 65, 264, 264), GuardedSpan(B * 65 * 264, F32, 64)
    pcm = lambda **kw: (lambda a: lib.tok_pix_class_matmul(a['x'], a['ldx'], a['m'], a['ldm'], B, n, a['k'], a['c'], 1.0, a['out'], st))(  # noqa: E731
        dict(dict(x=xg.ptr, ldx=264, m=mg.ptr, ldm=264, k=k, c=c, out=o32.ptr), **kw))
    cpe = lambda **kw: (lambda a: lib.tok_class_pix_expand(a['w'], a['m'], a['ldm'], B, n, a['k'], a['c'], 1.0, a['out'], a['ldo'], 0, st))(  # noqa: E731
        dict(dict(w=wg.ptr, m=mg.ptr, ldm=264, k=k, c=c, out=obf.ptr, ldo=264), **kw))
    wp = lambda **kw: (lambda a: lib.tok_weighted_pool(a['w'], a['x'], a['ldx'], B, n, a['k'], a['c'], 1.0, a['partial'], a['out'], a['ldo'], 0, st))(  # noqa: E731
        dict(dict(w=wg.ptr, x=xg.ptr, ldx=264, k=k, c=c, partial=part.ptr, out=obf.ptr, ldo=264), **kw))
    for kw in (dict(x=None), dict(m=None), dict(out=None), dict(k=65), dict(ldx=15), dict(ldm=15), dict(k=64, c=257)):
        refused(pcm(**kw), 'tok_pix_class_matmul', o32)
    for kw in (dict(w=None), dict(m=None), dict(out=None), dict(k=65), dict(ldm=15), dict(ldo=8), dict(ldo=20), dict(c=12, ldo=12), dict(k=64, c=257)):
        refused(cpe(**kw), 'tok_class_pix_expand', obf)
    for kw in (dict(w=None), dict(x=None), dict(partial=None), dict(out=None), dict(k=65), dict(ldx=15), dict(ldo=15), dict(k=41, c=250),
               dict(k=9, c=1100, ldx=1100, ldo=1100)):
        refused(wp(**kw), 'tok_weighted_pool', obf, part)
    assert (32 * (250 + 41) * 4 <= 65536 < 16 * (1100 + 9) * 4) and 41 * 250 == 10250 and 9 * 1100 <= 10240, 'each of the two rules refuses alone'
    assert lib.tok_weighted_pool_chunks(0) == ERR_INVALID and lib.tok_dwconv3x3_wgrad_blocks(0, 1) == ERR_INVALID

    lg = mat_in(d['m'])                       # any bf16 matrix
    refused(lib.tok_softmax_rows_f32(None, 4, 3, o32.ptr, st), 'tok_softmax_rows_f32', o32)
    refused(lib.tok_softmax_rows_f32(wg.ptr, 4, 3, None, st), 'tok_softmax_rows_f32')
    refused(lib.tok_softmax_rows_bwd_f32(None, wg.ptr, 4, 3, o32.ptr, st), 'tok_softmax_rows_bwd_f32', o32)
    refused(lib.tok_softmax_rows_bwd_f32(wg.ptr, wg.ptr, 4, 3, None, st), 'tok_softmax_rows_bwd_f32')
    for args in ((None, 8, 3), (lg.ptr, 8, 65), (lg.ptr, 2, 3)):
        refused(lib.tok_softmax_cols_fwd(args[0], args[1], B, n, args[2], 1.0, o32.ptr, st), 'tok_softmax_cols_fwd', o32)
    refused(lib.tok_softmax_cols_fwd(lg.ptr, 8, B, n, 3, 1.0, None, st), 'tok_softmax_cols_fwd')
    for args in ((None, wg.ptr, 3, obf.ptr, 8), (wg.ptr, None, 3, obf.ptr, 8), (wg.ptr, wg.ptr, 3, None, 8), (wg.ptr, wg.ptr, 65, obf.ptr, 72),
                 (wg.ptr, wg.ptr, 3, obf.ptr, 2)):
        refused(lib.tok_softmax_cols_bwd(args[0], args[1], B, n, args[2], 1.0, args[3], args[4], 0, st), 'tok_softmax_cols_bwd', obf)
    for args in ((None, wg.ptr, obf.ptr, 16, 16), (xg.ptr, None, obf.ptr, 16, 16), (xg.ptr, wg.ptr, None, 16, 16), (xg.ptr, wg.ptr, obf.ptr, 16, 8),
                 (xg.ptr, wg.ptr, obf.ptr, 12, 12)):
        refused(lib.tok_channel_scale(args[0], args[1], args[2], 0, B, n, args[3], args[4], st), 'tok_channel_scale', obf)

    rpi, heads = 5, 2
    x, y, m, _ = M.make_chan(B, rpi, heads, seed=1)
    qg, mm = mat_in(x, 72), mat_in(m)
    g32, gbf = mat_out(B * heads * HD, HD, dtype=F32), mat_out(B * rpi, 64, 72)
    gram = lambda x_=qg.ptr, y_=qg.ptr, ldx=72, ldy=72, mode=0, a_=None, o_=g32.ptr: lib.tok_chan_gram(  # noqa: E731
        x_, ldx, y_, ldy, rpi, B, heads, 1.0, mode, a_, o_, st)
    for kw in (dict(x_=None), dict(y_=None), dict(o_=None), dict(ldx=56), dict(ldy=68), dict(mode=3), dict(mode=-1), dict(mode=2)):
        refused(gram(**kw), 'tok_chan_gram', g32)
    app = lambda x_=qg.ptr, m_=mm.ptr, o_=gbf.ptr, ldx=72, ldo=72, images=B, hd=heads: lib.tok_chan_apply(  # noqa: E731
        x_, ldx, m_, 0, 1.0, rpi, images, hd, o_, ldo, st)
    for kw in (dict(x_=None), dict(m_=None), dict(o_=None), dict(ldx=56), dict(ldo=68), dict(images=65536, hd=1, ldx=32, ldo=32)):
        refused(app(**kw), 'tok_chan_apply', gbf)
    rs = mat_in(torch.ones(4))
    sra = lambda b_=qg.ptr, o_=gbf.ptr, rs_=None, rps=0, ld=72: lib.tok_scale_rows_add(None, b_, rs_, rps, o_, 0, B * rpi, ld, st)  # noqa: E731
    for kw in (dict(b_=None), dict(o_=None), dict(ld=68), dict(rs_=rs.ptr, rps=0)):
        refused(sra(**kw), 'tok_scale_rows_add', gbf)

    dd = M.make_dwconv(B, 3, 5, 20, seed=2)
    xd, wd = mat_in(dd['x'], 24), mat_in(dd['wt'])
    od, pd, dwo = mat_out(B * 15, 20, 24), GuardedSpan(6 * 20 * 10, F32, 64), mat_out(20, 9, dtype=F32)
    for args in ((None, wd.ptr, od.ptr, 24), (xd.ptr, None, od.ptr, 24), (xd.ptr, wd.ptr, None, 24), (xd.ptr, wd.ptr, od.ptr, 16), (xd.ptr, wd.ptr, od.ptr, 20)):
        refused(lib.tok_dwconv3x3(args[0], args[1], None, args[2], 0, 0, B, 3, 5, 20, args[3], st), 'tok_dwconv3x3', od)
    for args in ((None, xd.ptr, pd.ptr, dwo.ptr, 24), (xd.ptr, None, pd.ptr, dwo.ptr, 24), (xd.ptr, xd.ptr, None, dwo.ptr, 24), (xd.ptr, xd.ptr, pd.ptr, None, 24),
                 (xd.ptr, xd.ptr, pd.ptr, dwo.ptr, 16)):
        refused(lib.tok_dwconv3x3_wgrad(args[0], args[1], B, 3, 5, 20, args[4], args[2], args[3], None, 0, st), 'tok_dwconv3x3_wgrad', pd, dwo)
    kept(xg, mg, wg, lg, qg, mm, rs, xd, wd)


def test_misaligned_operands_are_refused():
    """Suspect 2.  The kernels of these six entries move 8 bf16 per access through a 16-byte vector type; the launchers checked the
    pitch (a multiple of 8) but not the base.  hipcc emits dwordx4 accesses on the strength of the type's alignment, and neither
    the ISA guide nor the programming guide of this project defines such an access at a 2-byte aligned address, so a base that is
    not 16-byte aligned is refused with TOK_ERR_INVALID (as tok_cast_bf16_f32, tok_upsample_ce_* and tok_global_attn_bias_fwd do);
    every caller in the engine passes allocation bases or offsets of whole 32-channel heads.  On the old library each of these
    calls was launched; none was run.  A refused call launches nothing: the operands are one element (2 bytes) or four elements
    (8 bytes) past a 16-byte boundary, inside buffers with room for them, and every output keeps its sentinels."""
    lib, st = _C.lib(), stream_ptr()
    rpi, heads, c = 5, 2, 64
    x, y, m, _ = M.make_chan(B, rpi, heads, seed=1)
    good, mm = mat_in(x), mat_in(m)
    g32 = mat_out(B * heads * HD, HD, dtype=F32)
    s = mat_in(torch.ones(B, c))
    w = mat_in(torch.rand(B, rpi, 3))
    wt = mat_in(torch.ones(c, 9))
    for off in (1, 4):
        bad_in, bad_out, good_out = mat_in(x, off=off), Mat(B * rpi, c, off=off), mat_out(B * rpi, c)
        assert bad_in.ptr % 16 == 2 * off and bad_out.ptr % 16 == 2 * off and good.ptr % 16 == 0
        refused(lib.tok_chan_gram(bad_in.ptr, c, good.ptr, c, rpi, B, heads, 1.0, 0, None, g32.ptr, st), 'tok_chan_gram', g32)
        refused(lib.tok_chan_gram(good.ptr, c, bad_in.ptr, c, rpi, B, heads, 1.0, 0, None, g32.ptr, st), 'tok_chan_gram', g32)
        refused(lib.tok_chan_apply(bad_in.ptr, c, mm.ptr, 0, 1.0, rpi, B, heads, good_out.ptr, c, st), 'tok_chan_apply', good_out)
        refused(lib.tok_chan_apply(good.ptr, c, mm.ptr, 0, 1.0, rpi, B, heads, bad_out.ptr, c, st), 'tok_chan_apply', bad_out)
        refused(lib.tok_scale_rows_add(bad_in.ptr, good.ptr, None, 0, good_out.ptr, 0, B * rpi, c, st), 'tok_scale_rows_add', good_out)
        refused(lib.tok_scale_rows_add(None, bad_in.ptr, None, 0, good_out.ptr, 0, B * rpi, c, st), 'tok_scale_rows_add', good_out)
        refused(lib.tok_scale_rows_add(None, good.ptr, None, 0, bad_out.ptr, 0, B * rpi, c, st), 'tok_scale_rows_add', bad_out)
        refused(lib.tok_class_pix_expand(w.ptr, good.ptr, c, B, rpi, 3, c, 1.0, bad_out.ptr, c, 0, st), 'tok_class_pix_expand', bad_out)
        refused(lib.tok_channel_scale(bad_in.ptr, s.ptr, good_out.ptr, 0, B, rpi, c, c, st), 'tok_channel_scale', good_out)
        refused(lib.tok_channel_scale(good.ptr, s.ptr, bad_out.ptr, 0, B, rpi, c, c, st), 'tok_channel_scale', bad_out)
        refused(lib.tok_dwconv3x3(bad_in.ptr, wt.ptr, None, good_out.ptr, 0, 0, B, 1, rpi, c, c, st), 'tok_dwconv3x3', good_out)
        refused(lib.tok_dwconv3x3(good.ptr, wt.ptr, None, bad_out.ptr, 0, 0, B, 1, rpi, c, c, st), 'tok_dwconv3x3', bad_out)
        kept(bad_in)
    kept(good, mm, s, w, wt)
