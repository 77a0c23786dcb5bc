"""The fused MLP (csrc/mlp_fused.hip: tok_mlp_fwd, tok_mlp_bwd_dx, tok_mlp_serves), the activation pair of csrc/layernorm.hip
(tok_act_fwd, tok_act_bwd) and the exact index kernels of csrc/transformer.hip (tok_cpb_bias_fwd / _bwd, tok_patch_merge) and
csrc/vit_embed.hip (tok_patch_gather, tok_vit_embed_fwd / _bwd, tok_rows_select) element by element against fp64 of the same inputs;
references, bounds with their derivations, input makers and case lists are in tests/mlp_rows_ref.py (tests/test_mlp_rows_ref.py holds
them to torch).  No element is excluded from a comparison except where a kernel's input is not finite and the operation has no value.

Every input sits behind NaN guards, every output in a sentinel-filled guarded buffer; after each call the guards are intact and every
owned element is written.  Every call runs twice and the two runs must be bit-identical, guards included.  Every MLP case names its
launch class and asserts it against the tile arithmetic (mlp_rows_ref.mlp_class), the wrap cases that they really exceed the 256
workgroups of the capped grid: there a workgroup walks several tiles, which for C = 192 and C = 384 (the non-prefetch forms: the
reload of the token rows after the epilogue, the ring and ledger state one tile hands to the next) nothing else in the suite reaches.
The wrap cases have rows of period P = 331 (built on the GPU): every output row r must have the bits of row r % P (checked on the
GPU), the first P rows are checked against fp64.

The MLP is checked stage by stage from the rows the kernel itself stored (pre, act = GELU(own pre), y from own act; dpre, dx from own
dpre), so every bound has one rounding in it; the forms that store less (no save, pre only, no dpre) must give the same bits.
The activations run over all 65536 bf16 bit patterns.

Decided here:
  1. tok_mlp_serves admitted rows * hidden * 2 < 2^32 while the kernels form 32-bit byte offsets for every row of the LAST TILE: with
     a ragged last tile that ends past 2^32 bytes the dropped rows' offsets wrap to small in-range ones and the SAVE stores (pre, act,
     dpre) would land in the first rows.  The rule is the tile-rounded count now (pinned host-side in tests/test_mlp_rows_ref.py,
     with no launch and no 4 GB buffer).
  2. tok_act_fwd / _bwd, tok_vit_embed_fwd (patch, out), tok_rows_select, tok_patch_merge and the bf16 operands of tok_mlp_fwd /
     tok_mlp_bwd_dx move 16 bytes per access, tok_patch_gather 8, from a base that was never checked: a misaligned base is refused
     with TOK_ERR_INVALID now (test_misaligned_operands_are_refused).
  3. tok_common.h said "a NaN input gives 0": true of a quiet NaN; a signalling one gives -5.6 Phi(-5.6) ~ -5e-8, the value of every
     x < -5.6 (v_med3_f32 clamps it to 5.6).  Finite either way; the comment and include/tok.h say so now, the kernel is unchanged,
     and test_act_fwd_gelu_every_bf16_input pins both.
The worst |err| / bound of every tensor is in profiles/mlp_rows_contract_parity_distances.json; the one-line kernel defects this
module was run against, with the module's timing, are in profiles/mlp_rows_contract_mutation_check.txt."""
import pytest
import torch

from helpers import A_BF, BF, ERR_INVALID, F32, GuardedSpan, Mat, U32, _INT_OF, cdiv, gin, gout, last_error
import mlp_rows_ref as M
from torchok_amd import _C
from torchok_amd.engine.core import stream_ptr

pytestmark = pytest.mark.gpu
TAG = 'mlp_rows_contract/'
I16 = torch.int16


@pytest.fixture(autouse=True, scope='module')
def _parity_record():
    """one line per kernel family and tensor: the worst |err| / bound over every case and variant of the family"""
    yield
    M.flush_record()


def mat_in(t, ld=None, off=0):
    """an input, its last axis the columns: NaN in the pads, in front and in both guards"""
    t = t.reshape(-1, t.shape[-1])
    return Mat(t.shape[0], t.shape[1], ld, dtype=t.dtype, init=t.cuda(), nan=True, off=off)


def mat_out(rows, cols, ld=None, dtype=BF, prior=None, off=0):
    """an output: sentinels everywhere, the owned elements holding `prior` under accumulate"""
    return Mat(rows, cols, ld, dtype=dtype, init=None if prior is None else prior.reshape(rows, cols).cuda(), off=off)


def kept(*ms):
    """inputs: guards (and pads, and the elements in front) still hold their NaN"""
    for m in ms:
        if isinstance(m, Mat):
            m.done('an input', finite=False)
        else:
            m.check('an input')


def written(span, what):
    span.check(what)
    assert int((span.view.view(_INT_OF[span.dtype]) == span.bits).sum()) == 0, f'{what}: owned elements never written'


def bits(*ms):
    out = []
    for m in ms:
        b = m.span.buf if isinstance(m, Mat) else m.buf
        out.append(b.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[b.element_size()]).clone())
    return out


def twice(run):
    """run() -> the output operands of one fresh call; two calls give the same bits"""
    a = bits(*run())
    second = run()
    for x, y in zip(a, bits(*second)):
        assert torch.equal(x, y), 'two runs of the same call differ'
    return second


def ok(rc, what):
    _C.check(rc, what)
    torch.cuda.synchronize()


def refused(rc, what):
    torch.cuda.synchronize()
    assert rc == ERR_INVALID, f'{what}: returned {rc}'
    assert last_error(), what


def same_bits(a, b, what):
    assert torch.equal(a.view(_INT_OF[a.dtype]), b.view(_INT_OF[b.dtype])), f'{what}: bits differ'


# ---- fused MLP ---------------------------------------------------------------------------------------------------------------------
class MlpCase:
    """the operands of one (rows, c): n base rows (all of them, or P under wrap) and their device copies with rows r = base[r % P]"""

    def __init__(self, rows, c, cls):
        self.rows, self.c, self.h, self.cls = rows, c, 4 * c, cls
        self.wrap = cls == 'wrap'
        self.n = M.P if self.wrap else rows
        self.d = M.make_mlp(c, self.n, seed=rows + c)
        self.idx = torch.arange(rows, device='cuda') % M.P if self.wrap else None
        lib = _C.lib()
        assert M.mlp_class(rows, c) == cls
        assert lib.tok_mlp_serves(rows, c, self.h) == 1 == M.mlp_serves(rows, c, self.h)
        assert (M.mlp_tiles(rows, c) > M.GRID_CAP) == self.wrap
        if self.wrap:
            assert rows > M.GRID_CAP * M.TILE[c] + M.TILE[c] and rows % 16 != 0        # a third tile for some workgroups, ragged end

    def rows_in(self, name):
        t = self.d[name].cuda()
        return mat_in(t[self.idx] if self.wrap else t)

    def prior(self):
        t = self.d['prior'].cuda()
        return t[self.idx] if self.wrap else t

    def own(self, m, what):
        """the first n rows of an output on the host; under wrap every row r first has to carry the bits of row r % P"""
        v = m.view
        if self.wrap:
            iv = v.view(I16)
            assert torch.equal(iv, iv[:M.P][self.idx]), f'{what}: a row differs from the row of its period'
        return v[:self.n].cpu()


@pytest.mark.parametrize('save', [False, True], ids=['nosave', 'save'])
@pytest.mark.parametrize('rows,c,cls', M.MLP_CASES)
def test_mlp_fwd(rows, c, cls, save):
    """save: pre, act and y stage by stage against fp64, then `pre` given with act = NULL: the same pre and y, act untouched.
    no save: y has the bits of the save form (and, from that form's act rows, is checked against fp64 again)"""
    lib, st = _C.lib(), stream_ptr()
    k = MlpCase(rows, c, cls)
    d, h = k.d, k.h
    assert M.reaches_the_tails(M.pre_ref(d)[0])
    xg, w1g, w2g = k.rows_in('x'), mat_in(d['w1']), mat_in(d['w2'])
    b1g, b2g = gin(d['b1'].cuda(), 64), gin(d['b2'].cuda(), 64)

    def form(pre_on, act_on):
        def run():
            yg, pg, ag = mat_out(rows, c), mat_out(rows, h), mat_out(rows, h)
            ok(lib.tok_mlp_fwd(xg.ptr, w1g.ptr, b1g.ptr, w2g.ptr, b2g.ptr, yg.ptr, pg.ptr if pre_on else None,
                               ag.ptr if act_on else None, rows, c, h, st), 'mlp_fwd')
            yg.done('y')
            pg.done('pre') if pre_on else pg.intact('pre')
            ag.done('act') if act_on else ag.intact('act')
            return [yg, pg, ag]
        return twice(run)
    yg, pg, ag = form(True, True)
    pre_own, act_own, y = k.own(pg, 'pre'), k.own(ag, 'act'), k.own(yg, 'y')
    tag = TAG + f'mlp_fwd c{c}'
    if save:
        M.check(tag, 'pre', pre_own, *M.pre_ref(d))
        M.check(tag, 'act', act_own, *M.act_ref(pre_own))
        M.check(tag, 'y', y, *M.y_ref(d, act_own))
        y2, p2, _ = form(True, False)
        same_bits(y2.view, yg.view, 'y of the pre-only form')
        same_bits(p2.view, pg.view, 'pre of the pre-only form')
    else:
        y0, _, _ = form(False, False)
        same_bits(y0.view, yg.view, 'y of the form that saves nothing')
        M.check(tag, 'y nosave', k.own(y0, 'y'), *M.y_ref(d, act_own))
    kept(xg, w1g, w2g, b1g, b2g)


@pytest.mark.parametrize('with_dpre', [True, False], ids=['dpre', 'nodpre'])
@pytest.mark.parametrize('acc', [0, 1])
@pytest.mark.parametrize('rows,c,cls', M.MLP_CASES)
def test_mlp_bwd_dx(rows, c, cls, acc, with_dpre):
    """dpre and dx stage by stage against fp64 (dx from the kernel's own dpre rows, fresh or added onto a prior); without dpre: dx has
    the bits of the form that stores it, and the dpre buffer is untouched"""
    lib, st = _C.lib(), stream_ptr()
    k = MlpCase(rows, c, cls)
    d, h = k.d, k.h
    assert M.reaches_the_tails(d['pre'])
    dyg, preg, w2g, w1g = k.rows_in('dy'), k.rows_in('pre'), mat_in(d['w2d']), mat_in(d['w1d'])
    prior = k.prior() if acc else None

    def form(dpre_on):
        def run():
            dxg, dpg = mat_out(rows, c, prior=prior), mat_out(rows, h)
            ok(lib.tok_mlp_bwd_dx(dyg.ptr, w2g.ptr, preg.ptr, w1g.ptr, dxg.ptr, acc, dpg.ptr if dpre_on else None, rows, c, h, st),
               'mlp_bwd_dx')
            dxg.done('dx')
            dpg.done('dpre') if dpre_on else dpg.intact('dpre')
            return [dxg, dpg]
        return twice(run)
    dxg, dpg = form(True)
    dpre_own, dx = k.own(dpg, 'dpre'), k.own(dxg, 'dx')
    tag = TAG + f'mlp_bwd_dx c{c}'
    if with_dpre:
        M.check(tag, 'dpre', dpre_own, *M.dpre_ref(d)[:2])
        M.check(tag, 'dx accumulated' if acc else 'dx', dx, *M.dx_ref(d, dpre_own, acc)[:2])
    else:
        dx0, _ = form(False)
        same_bits(dx0.view, dxg.view, 'dx of the form that stores no dpre')
        M.check(tag, 'dx nodpre', k.own(dx0, 'dx'), *M.dx_ref(d, dpre_own, acc)[:2])
    kept(dyg, preg, w2g, w1g)


def test_mlp_refusals():
    """act without pre; a geometry tok_mlp_serves does not admit; null pointers: TOK_ERR_INVALID, nothing written"""
    lib, st = _C.lib(), stream_ptr()
    rows, c = 77, 96
    h = 4 * c
    d = M.make_mlp(c, rows, seed=1)
    xg, w1g, w2g, preg = mat_in(d['x']), mat_in(d['w1']), mat_in(d['w2']), mat_in(d['pre'])
    b1g, b2g = gin(d['b1'].cuda(), 64), gin(d['b2'].cuda(), 64)
    yg, pg, ag = mat_out(rows, c), mat_out(rows, h), mat_out(rows, h)
    refused(lib.tok_mlp_fwd(xg.ptr, w1g.ptr, b1g.ptr, w2g.ptr, b2g.ptr, yg.ptr, None, ag.ptr, rows, c, h, st), 'act without pre')
    refused(lib.tok_mlp_fwd(xg.ptr, w1g.ptr, b1g.ptr, w2g.ptr, b2g.ptr, yg.ptr, pg.ptr, ag.ptr, rows, c, 2 * c, st), 'hidden = 2c')
    refused(lib.tok_mlp_fwd(xg.ptr, w1g.ptr, b1g.ptr, w2g.ptr, b2g.ptr, yg.ptr, pg.ptr, ag.ptr, 0, c, h, st), 'no rows')
    refused(lib.tok_mlp_fwd(None, w1g.ptr, b1g.ptr, w2g.ptr, b2g.ptr, yg.ptr, pg.ptr, ag.ptr, rows, c, h, st), 'x = NULL')
    refused(lib.tok_mlp_fwd(xg.ptr, w1g.ptr, None, w2g.ptr, b2g.ptr, yg.ptr, pg.ptr, ag.ptr, rows, c, h, st), 'b1 = NULL')
    refused(lib.tok_mlp_bwd_dx(xg.ptr, w1g.ptr, None, w2g.ptr, yg.ptr, 0, pg.ptr, rows, c, h, st), 'pre = NULL')
    refused(lib.tok_mlp_bwd_dx(xg.ptr, w1g.ptr, preg.ptr, w2g.ptr, yg.ptr, 0, pg.ptr, rows, 100, 400, st), 'c = 100')
    for m in (yg, pg, ag):
        m.intact('an output of a refused call')


# ---- activations -------------------------------------------------------------------------------------------------------------------
def _act_fwd(kind, x):
    lib, st = _C.lib(), stream_ptr()
    xg = gin(x.cuda(), 64)

    def run():
        og = gout(x.numel(), BF, 64)
        ok(lib.tok_act_fwd(kind, xg.ptr, og.ptr, x.numel(), st), 'act_fwd')
        og.check('out')
        return [og]
    og, = twice(run)
    xg.check('x')
    return og.value()


def _check_gelu_table(tag, x, out):
    fin = torch.isfinite(x.float())
    ref, bound = M.act_fwd_ref(1, x[fin])
    M.check(tag, 'gelu', out[fin], ref, bound)


def test_act_fwd_relu_every_bf16_input():
    """bit-exact to max(x, 0): a NaN gives 0 (fmaxf), -0 gives a zero of either sign"""
    x = M.bf16_table()
    out = _act_fwd(0, x)
    xf = x.float()
    want = torch.where(xf > 0, xf, torch.zeros_like(xf)).to(BF)
    assert torch.equal(out.float(), want.float())
    strict = x.view(I16) != torch.tensor(-32768, dtype=I16)               # every input but -0
    same_bits(out[strict], want[strict], 'relu')


def test_act_fwd_gelu_every_bf16_input():
    """every finite input within A_BF |ref| + 2^-20 max(1, |x|) of fp64 0.5 x (1 + erf(x / sqrt 2)); the special values pinned"""
    x = M.bf16_table()
    out = _act_fwd(1, x)
    _check_gelu_table(TAG + 'act_fwd', x, out)
    xf, of = x.float(), out.float()
    at = lambda b: of[b & 0xFFFF]          # noqa: E731  (output at a bit pattern)
    # a NaN input is dropped (tok_common.h): max(x, 0) gives 0, and v_med3_f32 clamps |x| to 0 for a quiet NaN (the result is 0, as
    # documented) and to 5.6 for a signalling one (the result is that of every x < -5.6, -5.6 Phi(-5.6) ~ -5e-8).  Arithmetic produces
    # quiet NaNs only.
    bits_ = torch.arange(65536)
    quiet = torch.isnan(xf) & ((bits_ & 0x0040) != 0)
    assert int(quiet.sum()) == 128 and bool((of[quiet] == 0).all()), 'a quiet NaN input gives 0'
    signalling = torch.isnan(xf) & ~quiet
    assert int(signalling.sum()) == 126 and bool((of[signalling] == at(0xFF80)).all()), 'a signalling NaN gives the value at the clamp'
    assert int(out.view(I16)[0x0000]) == 0 and float(at(0x8000)) == 0.0, '+0 -> +0, -0 -> a zero'
    assert float(at(0x7F80)) == float('inf'), '+inf -> +inf'
    # below -5.6 the tail is clamped: every such input, -inf included, gives the value at the clamp, -5.6 Phi(-5.6) ~ -6e-8
    low = of[(xf < -M.GELU_AMAX)]
    assert bool((low == at(0xFF80)).all()) and -M.G_ABS < float(at(0xFF80)) <= 0.0
    assert int(out.view(I16)[0x7F7F]) == 0x7F7F, 'the largest finite value is returned as it is'
    for b in (0x40B3, 0x40B4):             # 5.59375 and 5.625, the bf16 neighbours of +5.6: x Phi(x) rounds back to x
        assert int(out.view(I16)[b]) == b
    for b in (0xC0B3, 0xC0B4):             # the neighbours of -5.6
        assert -1.5e-7 < float(at(b)) < 0.0 and abs(float(at(b)) - float(M.gelu(x[b]))) <= M.G_ABS


@pytest.mark.parametrize('acc', [0, 1])
@pytest.mark.parametrize('kind', [0, 1, 2])
def test_act_bwd_every_bf16_input(kind, acc):
    """dx = bf16(g d(x) + prev), g = +-1, x every bf16 pattern; kind 1 at the finite x (GELU' of an infinity has no value), kinds 0 and
    2 at every x (NaN > 0 is false; the identity does not read x's value)"""
    lib, st = _C.lib(), stream_ptr()
    x = M.bf16_table()
    g, prev = M.make_act_bwd()
    xg, gg = gin(x.cuda(), 64), gin(g.cuda(), 64)

    def run():
        dg = gout(65536, BF, 64, init=prev.cuda() if acc else None)
        ok(lib.tok_act_bwd(kind, gg.ptr, xg.ptr, dg.ptr, acc, 65536, st), 'act_bwd')
        if kind == 1:
            dg.check('dx')
        else:
            written(dg, 'dx')
        return [dg]
    dg, = twice(run)
    out = dg.value()
    keep = torch.isfinite(x.float()) if kind == 1 else torch.ones(65536, dtype=torch.bool)
    ref, bound = M.act_bwd_ref(kind, g[keep], x[keep], prev[keep] if acc else None)
    M.check(TAG + f'act_bwd kind{kind}', 'dx accumulated' if acc else 'dx', out[keep], ref, bound)
    kept(xg, gg)


def test_act_second_trip_of_the_capped_grid():
    """65536 blocks x 256 threads x 8 elements is one trip; 2048 elements more make one block take a second one.  The 65536-pattern
    table repeated on the GPU: every 65536-block of the result equals the first, the first is checked against fp64"""
    lib, st = _C.lib(), stream_ptr()
    n = M.ACT_TRIP + 2048
    assert M.act_blocks(n) == 65536 and cdiv(n // 8, 256) == 65537
    reps = cdiv(n, 65536)
    x, (g, prev) = M.bf16_table(), M.make_act_bwd()
    rep = lambda t: t.cuda().repeat(reps)[:n]          # noqa: E731
    xg, gg = GuardedSpan(n, BF, 4096, init=rep(x), nan_guard=True), GuardedSpan(n, BF, 4096, init=rep(g), nan_guard=True)

    def periodic(span, what):
        iv = span.view.view(I16)
        first = iv[:65536]
        whole = n // 65536 * 65536
        assert torch.equal(iv[:whole].view(-1, 65536), first.expand(whole // 65536, 65536)), f'{what}: a block differs from the first'
        assert torch.equal(iv[whole:], first[:n - whole]), f'{what}: the second trip differs'
        return span.view[:65536].cpu()

    def fwd():
        og = GuardedSpan(n, BF, 4096)
        ok(lib.tok_act_fwd(1, xg.ptr, og.ptr, n, st), 'act_fwd')
        og.check('out')
        return [og]
    og, = twice(fwd)
    _check_gelu_table(TAG + 'act_fwd second trip', x, periodic(og, 'out'))
    del og

    def bwd():
        dg = GuardedSpan(n, BF, 4096, init=rep(prev))
        ok(lib.tok_act_bwd(1, gg.ptr, xg.ptr, dg.ptr, 1, n, st), 'act_bwd')
        dg.check('dx')
        return [dg]
    dg, = twice(bwd)
    out = periodic(dg, 'dx')
    keep = torch.isfinite(x.float())
    M.check(TAG + 'act_bwd second trip', 'dx accumulated', out[keep], *M.act_bwd_ref(1, g[keep], x[keep], prev[keep]))
    xg.check('x')
    gg.check('g')


def test_act_refusals():
    lib, st = _C.lib(), stream_ptr()
    x = M.bf16_table()[:64]
    xg, og = gin(x.cuda(), 64), gout(64, BF, 64)
    refused(lib.tok_act_fwd(1, xg.ptr, og.ptr, 60, st), 'count % 8')
    refused(lib.tok_act_fwd(1, xg.ptr, og.ptr, 0, st), 'count = 0')
    refused(lib.tok_act_fwd(2, xg.ptr, og.ptr, 64, st), 'kind 2 has no forward')
    refused(lib.tok_act_fwd(-1, xg.ptr, og.ptr, 64, st), 'kind -1')
    refused(lib.tok_act_fwd(1, None, og.ptr, 64, st), 'x = NULL')
    refused(lib.tok_act_fwd(1, xg.ptr, None, 64, st), 'out = NULL')
    refused(lib.tok_act_bwd(1, xg.ptr, xg.ptr, og.ptr, 0, 60, st), 'count % 8')
    refused(lib.tok_act_bwd(1, xg.ptr, xg.ptr, og.ptr, 0, 0, st), 'count = 0')
    refused(lib.tok_act_bwd(3, xg.ptr, xg.ptr, og.ptr, 0, 64, st), 'kind 3')
    refused(lib.tok_act_bwd(1, None, xg.ptr, og.ptr, 0, 64, st), 'dout = NULL')
    refused(lib.tok_act_bwd(1, xg.ptr, None, og.ptr, 0, 64, st), 'x = NULL')
    refused(lib.tok_act_bwd(1, xg.ptr, xg.ptr, None, 0, 64, st), 'dx = NULL')
    assert og.untouched()
    og.check('out')


# ---- SwinV2 continuous position bias ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ws,heads', M.CPB_CASES)
def test_cpb_bias(ws, heads):
    """forward against fp64 16 sigmoid(table[index]); backward against its ordered transpose with dbias stored plainly and transposed:
    the pad columns heads .. ld of dtable are written as zeros, the table rows no index names are 0"""
    lib, st = _C.lib(), stream_ptr()
    assert M.cpb_class(ws) == M.CPB_WS[ws]
    d = M.make_cpb(ws, heads, seed=ws + heads)
    n, rows, ld = d['n'], d['rows'], M.CPB_LD
    assert rows > int(d['index'].max()) + 1
    tg, ig = mat_in(d['table'], ld), gin(d['index'].cuda(), 64)

    def fwd():
        bg = gout(heads * n * n, F32, 64)
        ok(lib.tok_cpb_bias_fwd(tg.ptr, ld, ig.ptr, heads, n, bg.ptr, st), 'cpb_bias_fwd')
        written(bg, 'bias')
        return [bg]
    bg, = twice(fwd)
    M.check(TAG + 'cpb_bias_fwd', 'bias', bg.value().view(heads, n, n), *M.cpb_fwd_ref(d['table'], d['index']))
    for transposed in (0, 1):
        dg = gin(d['dbias'].cuda(), 64)

        def bwd():
            og = mat_out(rows, heads, ld)
            ok(lib.tok_cpb_bias_bwd(dg.ptr, transposed, tg.ptr, ld, ig.ptr, heads, n, rows, og.ptr, st), 'cpb_bias_bwd')
            og.done('dtable', zero_pads=True)
            return [og]
        og, = twice(bwd)
        ref, bound, _ = M.cpb_bwd_ref(d, transposed)
        M.check(TAG + 'cpb_bias_bwd', 'dtable transposed' if transposed else 'dtable', og.value(), ref, bound)
        assert bool((og.view[-M.CPB_SPARE_ROWS:] == 0).all()), 'rows no index names'
        dg.check('dbias')
    kept(tg, ig)


def test_cpb_refusals():
    lib, st = _C.lib(), stream_ptr()
    d = M.make_cpb(4, 3, seed=0)
    n, rows, ld = d['n'], d['rows'], M.CPB_LD
    tg, ig, dg = mat_in(d['table'], ld), gin(d['index'].cuda(), 64), gin(d['dbias'].cuda(), 64)
    bg, og = gout(3 * n * n, F32, 64), mat_out(rows, 3, ld)
    refused(lib.tok_cpb_bias_fwd(tg.ptr, 2, ig.ptr, 3, n, bg.ptr, st), 'ld < heads')
    refused(lib.tok_cpb_bias_fwd(tg.ptr, ld, ig.ptr, 0, n, bg.ptr, st), 'heads = 0')
    refused(lib.tok_cpb_bias_fwd(tg.ptr, ld, ig.ptr, 3, 0, bg.ptr, st), 'n_tokens = 0')
    refused(lib.tok_cpb_bias_fwd(None, ld, ig.ptr, 3, n, bg.ptr, st), 'table = NULL')
    refused(lib.tok_cpb_bias_fwd(tg.ptr, ld, None, 3, n, bg.ptr, st), 'index = NULL')
    refused(lib.tok_cpb_bias_fwd(tg.ptr, ld, ig.ptr, 3, n, None, st), 'bias = NULL')
    refused(lib.tok_cpb_bias_bwd(dg.ptr, 0, tg.ptr, 2, ig.ptr, 3, n, rows, og.ptr, st), 'ld < heads')
    refused(lib.tok_cpb_bias_bwd(dg.ptr, 0, tg.ptr, ld, ig.ptr, 0, n, rows, og.ptr, st), 'heads = 0')
    refused(lib.tok_cpb_bias_bwd(dg.ptr, 0, tg.ptr, ld, ig.ptr, 3, 0, rows, og.ptr, st), 'n_tokens = 0')
    refused(lib.tok_cpb_bias_bwd(dg.ptr, 0, tg.ptr, ld, ig.ptr, 3, n, 0, og.ptr, st), 'table_rows = 0')
    refused(lib.tok_cpb_bias_bwd(None, 0, tg.ptr, ld, ig.ptr, 3, n, rows, og.ptr, st), 'dbias = NULL')
    refused(lib.tok_cpb_bias_bwd(dg.ptr, 0, None, ld, ig.ptr, 3, n, rows, og.ptr, st), 'table = NULL')
    refused(lib.tok_cpb_bias_bwd(dg.ptr, 0, tg.ptr, ld, None, 3, n, rows, og.ptr, st), 'index = NULL')
    refused(lib.tok_cpb_bias_bwd(dg.ptr, 0, tg.ptr, ld, ig.ptr, 3, n, rows, None, st), 'dtable = NULL')
    assert bg.untouched()
    og.intact('dtable')


# ---- permutations ------------------------------------------------------------------------------------------------------------------
def _merge(src, b, h, w, c, inverse):
    lib, st = _C.lib(), stream_ptr()
    sg = gin(src.reshape(-1), 256)

    def run():
        og = gout(src.numel(), BF, 256)
        ok(lib.tok_patch_merge(sg.ptr, og.ptr, b, h, w, c, inverse, st), 'patch_merge')
        written(og, 'dst')
        return [og]
    og, = twice(run)
    sg.check('src')
    return og.view


@pytest.mark.parametrize('b,h,w,c', M.MERGE_CASES + [M.MERGE_BIG], ids=lambda v: str(v))
def test_patch_merge(b, h, w, c):
    """the forward is PatchMerging's cat(x0, x1, x2, x3) bit for bit, the inverse undoes it bit for bit; the last case needs more than
    the 65536 blocks of the capped grid (a second trip) and is compared on the GPU"""
    big = (b, h, w, c) == M.MERGE_BIG
    assert (b * h * w * c // 8 > 65536 * 256) == big
    x = M.bit_pattern(b * h * w * c, seed=h + w + c, device='cuda').view(b, h, w, c)
    want = M.patch_merge_ref(x).contiguous()
    merged = _merge(x, b, h, w, c, 0)
    same_bits(merged, want.reshape(-1), 'merged')
    del merged
    back = _merge(want, b, h, w, c, 1)
    same_bits(back, x.reshape(-1), 'the inverse of the merged rows')
    if not big:
        # the inverse on rows that are no forward result: element (y, x, q, c) goes to (2y + (q & 1), 2x + (q >> 1), c)
        y = M.bit_pattern(b * h * w * c, seed=1, device='cuda').view(b, h // 2, w // 2, 4, c)
        z = torch.empty(b, h, w, c, dtype=BF, device='cuda')
        for q in range(4):
            z[:, (q & 1)::2, (q >> 1)::2] = y[:, :, :, q]
        same_bits(_merge(y, b, h, w, c, 1), z.reshape(-1), 'inverse')


@pytest.mark.parametrize('n,h,w,p', M.GATHER_CASES)
def test_patch_gather(n, h, w, p):
    lib, st = _C.lib(), stream_ptr()
    img = M.bit_pattern(n * h * w * 4, seed=h + w + p).view(n, h, w, 4)
    ig = gin(img.cuda().reshape(-1), 256)

    def run():
        og = gout(img.numel(), BF, 256)
        ok(lib.tok_patch_gather(ig.ptr, n, h, w, p, og.ptr, st), 'patch_gather')
        written(og, 'rows')
        return [og]
    og, = twice(run)
    same_bits(og.value(), M.patch_gather_ref(img, p).reshape(-1), 'rows')
    ig.check('img')


def test_permutation_refusals():
    lib, st = _C.lib(), stream_ptr()
    x = M.bit_pattern(2 * 6 * 6 * 16, seed=0).cuda()
    sg, og = gin(x, 256), gout(x.numel(), BF, 256)
    refused(lib.tok_patch_merge(sg.ptr, og.ptr, 2, 5, 6, 16, 0, st), 'odd H')
    refused(lib.tok_patch_merge(sg.ptr, og.ptr, 2, 6, 5, 16, 0, st), 'odd W')
    refused(lib.tok_patch_merge(sg.ptr, og.ptr, 2, 6, 6, 12, 0, st), 'C % 8')
    refused(lib.tok_patch_merge(None, og.ptr, 2, 6, 6, 16, 0, st), 'src = NULL')
    refused(lib.tok_patch_gather(sg.ptr, 2, 6, 9, 2, og.ptr, st), 'w % p')
    refused(lib.tok_patch_gather(sg.ptr, 2, 9, 6, 2, og.ptr, st), 'h % p')
    refused(lib.tok_patch_gather(sg.ptr, 2, 2, 2, 4, og.ptr, st), 'p > h')
    assert og.untouched()
    og.check('dst')


# ---- ViT token assembly ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b', M.EMBED_B)
@pytest.mark.parametrize('nec', [0, 1])
@pytest.mark.parametrize('has_cls', [0, 1])
def test_vit_embed(has_cls, nec, b):
    """forward: one add, one bf16 rounding.  backward: d(pos) and d(cls) fresh and accumulated; each NULL on its own, the other with the
    bits it has when both are given; both NULL: accepted, nothing to write"""
    lib, st = _C.lib(), stream_ptr()
    for p in M.EMBED_P:
        for dm in M.EMBED_D:
            e = M.make_embed(b, p, dm, has_cls, seed=b + p + dm)
            t = e['t']
            pg, posg = mat_in(e['patch']), gin(e['pos'].cuda(), 64)
            cg = gin(e['cls'].cuda(), 64) if has_cls else None

            def fwd():
                og = mat_out(b * t, dm)
                ok(lib.tok_vit_embed_fwd(pg.ptr, posg.ptr, cg.ptr if has_cls else None, b, p, dm, nec, og.ptr, st), 'vit_embed_fwd')
                og.done('out')
                return [og]
            og, = twice(fwd)
            ref, slack = M.embed_fwd_ref(e, nec)
            M.check(TAG + 'vit_embed_fwd', 'out', og.value().view(b, t, dm), ref, A_BF * ref.abs() + slack)
            kept(pg, posg)

            dg = mat_in(e['dout'])
            dpos, dcls, sp, sc = M.embed_bwd_ref(e, nec)
            rows_l = dpos.shape[0]
            assert rows_l == (p if nec else t)

            def bwd(pos_on, cls_on, acc):
                def run():
                    pos_o = gout(rows_l * dm, F32, 64, init=e['dpos_prior'][:rows_l].cuda() if acc and pos_on else None)
                    cls_o = gout(dm, F32, 64, init=e['dcls_prior'].cuda() if acc and cls_on else None)
                    ok(lib.tok_vit_embed_bwd(dg.ptr, b, p, dm, has_cls, nec, pos_o.ptr if pos_on else None, acc,
                                             cls_o.ptr if cls_on else None, acc, st), 'vit_embed_bwd')
                    for o, on, what in ((pos_o, pos_on, 'dpos'), (cls_o, cls_on, 'dcls')):
                        o.check(what)
                        if on:
                            written(o, what)
                        else:
                            assert o.untouched(), f'{what}: written though NULL was passed'
                    return [pos_o, cls_o]
                return twice(run)
            both = {}
            for acc in (0, 1):
                pos_o, cls_o = both[acc] = bwd(True, bool(has_cls), acc)
                pp = e['dpos_prior'][:rows_l].double() if acc else 0.0
                M.check(TAG + 'vit_embed_bwd', 'dpos accumulated' if acc else 'dpos', pos_o.value().view(rows_l, dm), dpos + pp,
                        sp + (U32 * pp.abs() if acc else 0.0))
                if has_cls:
                    cp = e['dcls_prior'].double() if acc else 0.0
                    M.check(TAG + 'vit_embed_bwd', 'dcls accumulated' if acc else 'dcls', cls_o.value(), dcls + cp,
                            sc + (U32 * cp.abs() if acc else 0.0))
            for acc in (0, 1):
                if has_cls:
                    _, cls_only = bwd(False, True, acc)
                    same_bits(cls_only.view, both[acc][1].view, 'dcls with dpos = NULL')
                    pos_only, _ = bwd(True, False, acc)
                    same_bits(pos_only.view, both[acc][0].view, 'dpos with dcls = NULL')
                bwd(False, False, acc)
            kept(dg)


def test_vit_embed_refusals():
    lib, st = _C.lib(), stream_ptr()
    e = M.make_embed(2, 5, 24, 0, seed=0)
    pg, posg, dg = mat_in(e['patch']), gin(e['pos'].cuda(), 64), mat_in(e['dout'])
    og, pos_o, cls_o = mat_out(2 * 6, 24), gout(6 * 24, F32, 64), gout(24, F32, 64)
    refused(lib.tok_vit_embed_bwd(dg.ptr, 2, 5, 24, 0, 0, pos_o.ptr, 0, cls_o.ptr, 0, st), 'dcls with has_cls = 0')
    refused(lib.tok_vit_embed_bwd(dg.ptr, 2, 5, 20, 0, 0, pos_o.ptr, 0, None, 0, st), 'd % 8')
    refused(lib.tok_vit_embed_bwd(None, 2, 5, 24, 0, 0, pos_o.ptr, 0, None, 0, st), 'dout = NULL')
    refused(lib.tok_vit_embed_fwd(pg.ptr, posg.ptr, None, 2, 5, 20, 0, og.ptr, st), 'd % 8')
    refused(lib.tok_vit_embed_fwd(pg.ptr, posg.ptr, None, 0, 5, 24, 0, og.ptr, st), 'batch = 0')
    refused(lib.tok_vit_embed_fwd(pg.ptr, None, None, 2, 5, 24, 0, og.ptr, st), 'pos = NULL')
    og.intact('out')
    assert pos_o.untouched() and cls_o.untouched()


@pytest.mark.parametrize('d', [8, 24])
@pytest.mark.parametrize('t,first,count', M.SELECT_CASES)
def test_rows_select(t, first, count, d):
    """dir 0: the rows, bit for bit.  dir 1 fresh: the selected rows bit for bit, the others +0.  dir 1 accumulated: one rounding on the
    selected rows, the others keep their bits"""
    lib, st = _C.lib(), stream_ptr()
    b = 2
    g = M.gen(t + first + count + d)
    src = M.bf(torch.randn(b * t, d, generator=g))
    sel = M.bf(torch.randn(b * count, d, generator=g))
    prior = M.bf(torch.randn(b * t, d, generator=g))
    sg, selg = mat_in(src), mat_in(sel)

    def gather():
        og = mat_out(b * count, d)
        ok(lib.tok_rows_select(sg.ptr, b, t, first, count, d, og.ptr, 0, 0, st), 'rows_select')
        og.done('dst')
        return [og]
    og, = twice(gather)
    same_bits(og.value(), M.rows_select_ref(src, b, t, first, count, d), 'dir 0')

    def scatter(acc):
        def run():
            og = mat_out(b * t, d, prior=prior if acc else None)
            ok(lib.tok_rows_select(selg.ptr, b, t, first, count, d, og.ptr, 1, acc, st), 'rows_select')
            og.done('dst')
            return [og]
        return twice(run)[0].value().view(b, t, d)
    inside = torch.zeros(t, dtype=torch.bool)
    inside[first:first + count] = True
    fresh = scatter(0)
    same_bits(fresh[:, inside], sel.view(b, count, d), 'dir 1: the selected rows')
    assert bool((fresh[:, ~inside].reshape(-1).view(I16) == 0).all()), 'dir 1: the other rows are +0'
    accd = scatter(1)
    pv = prior.view(b, t, d)
    same_bits(accd[:, ~inside], pv[:, ~inside], 'dir 1 accumulated: the other rows')
    ref = pv[:, inside].double() + sel.view(b, count, d).double()
    M.check(TAG + 'rows_select', 'dst accumulated', accd[:, inside], ref, A_BF * ref.abs())
    kept(sg, selg)


def test_rows_select_refusals():
    lib, st = _C.lib(), stream_ptr()
    src = M.bf(torch.randn(2 * 6, 8, generator=M.gen(0)))
    sg, og = mat_in(src), mat_out(2 * 6, 8)
    refused(lib.tok_rows_select(sg.ptr, 2, 6, 3, 4, 8, og.ptr, 0, 0, st), 'first + count > t')
    refused(lib.tok_rows_select(sg.ptr, 2, 6, 1, 4, 8, og.ptr, 2, 0, st), 'dir = 2')
    refused(lib.tok_rows_select(sg.ptr, 2, 6, 1, 4, 12, og.ptr, 0, 0, st), 'd % 8')
    refused(lib.tok_rows_select(sg.ptr, 2, 6, -1, 4, 8, og.ptr, 0, 0, st), 'first < 0')
    og.intact('dst')


# ---- alignment ---------------------------------------------------------------------------------------------------------------------
def test_misaligned_operands_are_refused():
    """the entries that move 16 bytes per access refuse a base 8 bytes off (4 bf16 elements: the pitch rule alone would pass it),
    tok_patch_gather (8 bytes per access) a base 4 bytes off while it takes one 8 bytes off; every buffer has its full size, and a
    refused call launches nothing: the outputs keep their sentinels"""
    lib, st = _C.lib(), stream_ptr()
    outs = []

    def o(rows, cols, off=0):
        outs.append(mat_out(rows, cols, off=off))
        return outs[-1]
    x = M.bf(torch.randn(64, 8, generator=M.gen(0)))
    a, a4 = mat_in(x), mat_in(x, off=4)
    # activations
    refused(lib.tok_act_fwd(1, a4.ptr, o(64, 8).ptr, 512, st), 'act_fwd x')
    refused(lib.tok_act_fwd(1, a.ptr, o(64, 8, 4).ptr, 512, st), 'act_fwd out')
    refused(lib.tok_act_bwd(1, a4.ptr, a.ptr, o(64, 8).ptr, 0, 512, st), 'act_bwd dout')
    refused(lib.tok_act_bwd(1, a.ptr, a4.ptr, o(64, 8).ptr, 0, 512, st), 'act_bwd x')
    refused(lib.tok_act_bwd(1, a.ptr, a.ptr, o(64, 8, 4).ptr, 0, 512, st), 'act_bwd dx')
    # token assembly and row selection: 4 images of 16 rows
    pos = gin(torch.randn(16, 8, generator=M.gen(1)).cuda(), 64)
    refused(lib.tok_vit_embed_fwd(a4.ptr, pos.ptr, None, 4, 16, 8, 0, o(64, 8).ptr, st), 'vit_embed_fwd patch')
    refused(lib.tok_vit_embed_fwd(a.ptr, pos.ptr, None, 4, 16, 8, 0, o(64, 8, 4).ptr, st), 'vit_embed_fwd out')
    for direction in (0, 1):
        refused(lib.tok_rows_select(a4.ptr, 4, 16, 0, 16, 8, o(64, 8).ptr, direction, 0, st), 'rows_select src')
        refused(lib.tok_rows_select(a.ptr, 4, 16, 0, 16, 8, o(64, 8, 4).ptr, direction, 0, st), 'rows_select dst')
    # patch merge (1, 8, 8, 8) and patch gather (1, 8, 16, p = 2): 512 elements each
    for inverse in (0, 1):
        refused(lib.tok_patch_merge(a4.ptr, o(64, 8).ptr, 1, 8, 8, 8, inverse, st), 'patch_merge src')
        refused(lib.tok_patch_merge(a.ptr, o(64, 8, 4).ptr, 1, 8, 8, 8, inverse, st), 'patch_merge dst')
    a2 = mat_in(x, off=2)
    refused(lib.tok_patch_gather(a2.ptr, 1, 8, 16, 2, o(64, 8).ptr, st), 'patch_gather img')
    refused(lib.tok_patch_gather(a.ptr, 1, 8, 16, 2, o(64, 8, 2).ptr, st), 'patch_gather rows')
    for m in outs:
        m.intact('an output of a refused call')
    g8 = mat_out(64, 8, off=4)
    ok(lib.tok_patch_gather(a4.ptr, 1, 8, 16, 2, g8.ptr, st), 'patch_gather, 8-byte aligned')
    same_bits(g8.value().reshape(-1), M.patch_gather_ref(x.view(1, 8, 16, 4), 2).reshape(-1), 'rows from an 8-byte aligned base')
    g8.done('rows')
    # the fused MLP: every bf16 operand in turn
    outs.clear()
    rows, c = 16, 96
    h = 4 * c
    d = M.make_mlp(c, rows, seed=3)
    b1g, b2g = gin(d['b1'].cuda(), 64), gin(d['b2'].cuda(), 64)
    ins = {k: (mat_in(d[k]), mat_in(d[k], off=4)) for k in ('x', 'w1', 'w2', 'dy', 'w2d', 'pre', 'w1d')}
    for bad in ('x', 'w1', 'w2', 'y', 'pre', 'act'):
        p_ = {k: ins[k][k == bad].ptr for k in ('x', 'w1', 'w2')}
        yg, pg, ag = o(rows, c, 4 * (bad == 'y')), o(rows, h, 4 * (bad == 'pre')), o(rows, h, 4 * (bad == 'act'))
        refused(lib.tok_mlp_fwd(p_['x'], p_['w1'], b1g.ptr, p_['w2'], b2g.ptr, yg.ptr, pg.ptr, ag.ptr, rows, c, h, st), f'mlp_fwd {bad}')
    for bad in ('dy', 'w2d', 'pre', 'w1d', 'dx', 'dpre'):
        p_ = {k: ins[k][k == bad].ptr for k in ('dy', 'w2d', 'pre', 'w1d')}
        dxg, dpg = o(rows, c, 4 * (bad == 'dx')), o(rows, h, 4 * (bad == 'dpre'))
        refused(lib.tok_mlp_bwd_dx(p_['dy'], p_['w2d'], p_['pre'], p_['w1d'], dxg.ptr, 0, dpg.ptr, rows, c, h, st), f'mlp_bwd_dx {bad}')
    for m in outs:
        m.intact('an output of a refused call')
