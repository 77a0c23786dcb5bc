"""fp64 reference of the softmax attention that csrc/attn_tile.h serves, with the element-wise error bound of every result: the
oracle of tests/test_attn_tile_contract_gpu.py and of the tightened tests/test_global_attn_contract_gpu.py.  One module for both
row addressings: dense rows (ViT / BEiT, head_dim 64: `dense_units`) and window rows, local and shared-query (GCViT, head_dim 32:
`window_units`, `window_index`).  Everything is computed in the unit layout [units][heads][N][head_dim]; the adapters move token
rows into it and the kernels' results with them, so no comparison depends on a second restatement of the addressing.

    S = scale Q K^T + bias      P = softmax(S)      O = P V      lse = logsumexp(S)
    dP = dO V^T                 delta = rowsum(dO o O)           dS = P o (dP - delta)
    dQ = scale dS K             dK = scale dS^T Q                dV = P^T dO        dbias = sum over the units of dS
    shared query: unit u takes Q of image qimg[u];  d(q_global)[img] = sum over {u: qimg[u] == img} of dQ_u

Bounds.  Every bound is element-wise, |kernel - ref| <= a |ref| + b mag + 2^-90 max(mag); `Ref.bounds[name]` is (a, b, mag).
u = 2^-8 is one bf16 rounding (8 significant bits, round to nearest even: f2bf), e = 2^-24 one fp32 rounding, nt the number of
64-key tiles.  The last term is the flush floor: fp32 and bf16 flush below 2^-126, so a term more than 2^-90 below the largest of its tensor (a P of
e^-100 in the sharp cases) is held to that absolute size and not to a relative one.  The derivation follows the rounding points
of attn_tile.h:

 logits    t = fma(s, scale log2e, bias log2e rounded).  s is the MFMA's fp32 sum of exact bf16 products, taken to err by at most
           4 e sum|q||k| (HD / 16 roundings of the running magnitude; the accumulation inside an MFMA is not documented, this is the
           assumption of the derivation); the two constants, the bias product and the fma add 4 more roundings of magnitudes that
           L[i][j] = scale sum_d |q||k| + |bias| (nats) dominates: 8 in the forward and in dQ / dK / dV, 9 in the dense d(bias)
           (below); 10 is used.  The subtraction t - m before exp2 rounds e |t - m|; exp2f and log2f are held to 2 ulp = 4 e.
           Together  tau[i][j] = e (10 L[i][j] + |S[i][j] - max_j S[i]| + 4)  bounds the relative error of one unnormalised
           probability; it is per element, because a bias of -3e4 on a masked key (L = 3e4) must not loosen the row's live keys.
 row sum   l is an fp32 sum of unrounded terms: 4 sequential adds and a 16-lane tree (8 e), and per tile one exp2f (alpha), one
           product and one add (6 e): relative error  lam[i] = sum_j P tau + e (6 nt + 8).  An error of the running maximum cancels
           in lse and in P.
 lse       (m + log2 l) ln2: lam, the log2f, the add and the product (a rounded constant): |err| <= 8 e |lse| + lam.  The row sum is
           fp32, so no bf16 rounding enters: a few fp32 ulps of |lse| and of the logits that carry weight.
 out       P is rounded to bf16 before the P V MFMA (u P |V|), each P carries rho = tau + lam, the accumulator is rescaled and added
           to once per tile ((4 nt + 4) e), the result is rounded to bf16 (u |computed|):
           |err| <= u |O| + u (1 + 2^-6) sum_j P (1 + (rho + (4 nt + 4) e) / u) |V|.
 backward  P is recomputed as exp2(fma(s, scale log2e, -(fma(-bias, log2e, lse log2e rounded)))): lse log2e is rounded once, so
           rb = tau + (bound of lse) + 8 e |lse| bounds its relative error (the dense d(bias) forms lse - bias log2e in two
           roundings where the others have one fma: the 9th of the count in tau).
 delta     dense family: rowsum(dO o O) of the STORED bf16 O: e_delta = sum_d |dO| (bound of out) + 64 e sum_d |dO||O|.
           windowed family: rowsum(P o dP) of the unrounded P in fp32: e_delta = sum_j (rb + (8 nt + 16) e) P (|dO||V|^T).
 dS        (P^ - P)(dP - delta) + P^ (err dP - err delta) and two fp32 roundings:
           E = rb |dS| + P (e_delta + 4 e |dO||V|^T) (1 + rb) + 2 e |dS|.
 dq, dk    dS is rounded to bf16 before its MFMA (u |dS^|), accumulated over the tiles and rounded to bf16:
           G = u |dS| + (1 + u) E + (4 nt + 4) e |dS|;  |err| <= u |ref| + (1 + 2^-6) scale (G |K|  resp.  G^T |Q|).
 dv        P^ rounded to bf16: Gv = P (u + (1 + u) rb + (4 nt + 4) e);  |err| <= u |ref| + (1 + 2^-6) Gv^T |dO|.
 dq_global the workgroup keeps the fp32 sum over its windows in the accumulators and rounds once: the per-window terms add up.
 dbias     dS stays fp32 and is summed by fmaf over the units of a chunk, the chunks are folded in fp32:
           |err| <= sum_u E + (U + chunks + 2) e sum_u |dS|.  No bf16 rounding of dS enters; in the dense family the u of the
           stored O is inside E through e_delta.
No term had to be measured."""
import torch

U16 = 2.0 ** -8        # one bf16 rounding
E32 = 2.0 ** -24       # one fp32 rounding
FLOOR = 2.0 ** -90     # flush floor, relative to the largest magnitude of the tensor
TL = 64                # tokens per tile (csrc/attn_tile.h)
SCALE = {64: 0.125, 32: 32 ** -0.5}


def cdiv(a, b):
    return -(-a // b)


# ---- addressing ------------------------------------------------------------------------------------------------------------------
def dense_units(rows, b, n, heads, parts, hd=64):
    """token rows [b*n][parts*heads*hd] -> `parts` tensors [b][heads][n][hd] (views)"""
    t = rows.reshape(b, n, parts, heads, hd).permute(2, 0, 3, 1, 4)
    return tuple(t[i] for i in range(parts))


def dense_rows(*units):
    """the inverse: tensors [b][heads][n][hd] -> rows [b*n][len(units)*heads*hd]"""
    b, heads, n, hd = units[0].shape
    return torch.stack([t.transpose(1, 2) for t in units], 2).reshape(b * n, len(units) * heads * hd).contiguous()


def window_index(b, h, w, ws):
    """int64 [b * nW][N]: the token row of token t of window u (u image-major: img * nW + wy * nWx + wx)"""
    idx = torch.arange(b * h * w).view(b, h // ws, ws, w // ws, ws)
    return idx.permute(0, 1, 3, 2, 4).reshape(-1, ws * ws)


def window_units(rows, geo, parts, hd=32):
    """token rows [B*H*W][parts*heads*hd] -> `parts` tensors [B*nW][heads][N][hd]"""
    b, h, w, heads, ws = geo
    xw = rows[window_index(b, h, w, ws)]
    t = xw.reshape(xw.shape[0], ws * ws, parts, heads, hd).permute(2, 0, 3, 1, 4)
    return tuple(t[i] for i in range(parts))


def window_rows(geo, *units):
    """the inverse: tensors [B*nW][heads][N][hd] -> token rows [B*H*W][len(units)*heads*hd]"""
    b, h, w, heads, ws = geo
    idx = window_index(b, h, w, ws).reshape(-1)
    bw, _, n, hd = units[0].shape
    flat = torch.stack([t.transpose(1, 2) for t in units], 2).reshape(bw * n, len(units) * heads * hd)
    out = torch.zeros(b * h * w, flat.shape[1], dtype=flat.dtype)
    out[idx] = flat
    return out


def query_image(units, batch):
    """the image whose q_global unit u reads: u mod B (the reference's `repeat` tiles image-minor)"""
    return torch.arange(units) % batch


def dbias_chunks(units, n, heads, max_chunks):
    """Python restatement of dbias_per_chunk (csrc/attn_tile.h) -> (units per chunk, chunks): 2048 workgroups wanted, at most
    max_chunks partial tables (64 dense, 128 windowed), never more chunks than units"""
    tiles = cdiv(n, TL) ** 2 * heads
    chunks = min(cdiv(2048, tiles), max_chunks, units)
    per = cdiv(units, chunks)
    return per, cdiv(units, per)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
class Ref:
    """fp64 forward / backward in the unit layout.  q [Uq][H][N][D], k / v / dout [U][H][N][D] (any float dtype, taken exactly),
    bias [H][N][N] or None; qimg (int64 [U]) makes the query shared: unit u reads q[qimg[u]] and `dq_global` [Uq][H][N][D] is
    returned in place of `dq`.  family: 'dense' | 'windowed' (where delta comes from, see the module docstring).
    Results: out, lse, dq | dq_global, dk, dv, dbias (None without a bias); bounds[name] = (a, b, mag)."""

    def __init__(self, q, k, v, dout, bias=None, qimg=None, family='dense', chunks=1):
        assert family in ('dense', 'windowed')
        U, H, N, D = k.shape
        sc, nt = SCALE[D], cdiv(N, TL)
        q, k, v, go = q.double(), k.double(), v.double(), dout.double()
        qu = q if qimg is None else q[qimg]
        s = (qu @ k.transpose(-2, -1)) * sc
        L = (qu.abs() @ k.abs().transpose(-2, -1)) * sc
        if bias is not None:
            s = s + bias.double().unsqueeze(0)
            L = L + bias.double().abs().unsqueeze(0)
        self.s = s
        self.lse = torch.logsumexp(s, -1)
        p = torch.exp(s - self.lse.unsqueeze(-1))
        self.p = p
        self.out = p @ v
        ka, va, ga, qa = k.abs(), v.abs(), go.abs(), qu.abs()
        tau = E32 * (10 * L + (s - s.amax(-1, keepdim=True)).abs() + 4)
        del L
        lam = (p * tau).sum(-1) + E32 * (6 * nt + 8)
        acc = (4 * nt + 4) * E32
        self.bounds = {'lse': (8 * E32, 1.0, lam)}
        b_lse = 8 * E32 * self.lse.abs() + lam
        m_out = (p * (1 + (tau + lam.unsqueeze(-1) + acc) / U16)) @ va
        self.bounds['out'] = (U16, U16 * (1 + 2.0 ** -6), m_out)
        b_out = self.bound('out')
        # backward
        rb = tau + (b_lse + 8 * E32 * self.lse.abs()).unsqueeze(-1)
        del tau
        dp = go @ v.transpose(-2, -1)
        dpa = ga @ va.transpose(-2, -1)
        delta = (go * self.out).sum(-1)
        if family == 'dense':
            e_delta = (ga * b_out).sum(-1) + 64 * E32 * (ga * self.out.abs()).sum(-1)
        else:
            e_delta = ((rb + (8 * nt + 16) * E32) * p * dpa).sum(-1)
        ds = p * (dp - delta.unsqueeze(-1))
        del dp
        dsa = ds.abs()
        err = rb * dsa + p * (e_delta.unsqueeze(-1) + 4 * E32 * dpa) * (1 + rb) + 2 * E32 * dsa
        del dpa
        g = (U16 * dsa + (1 + U16) * err + acc * dsa) * (sc * (1 + 2.0 ** -6) / U16)
        dq, m_dq = sc * (ds @ k), g @ ka
        self.dk = sc * (ds.transpose(-2, -1) @ qu)
        self.bounds['dk'] = (U16, U16, g.transpose(-2, -1) @ qa)
        del g
        self.dv = p.transpose(-2, -1) @ go
        gv = p * ((U16 + (1 + U16) * rb + acc) * ((1 + 2.0 ** -6) / U16))
        self.bounds['dv'] = (U16, U16, gv.transpose(-2, -1) @ ga)
        del gv, rb
        if qimg is None:
            self.dq, self.dq_global = dq, None
            self.bounds['dq'] = (U16, U16, m_dq)
        else:
            self.dq = None
            self.dq_global = torch.zeros_like(q).index_add_(0, qimg, dq)
            self.bounds['dq_global'] = (U16, U16, torch.zeros_like(q).index_add_(0, qimg, m_dq))
        self.dbias = None
        if bias is not None:
            self.dbias = ds.sum(0)
            self.bounds['dbias'] = (0.0, 1.0, err.sum(0) + (U + chunks + 2) * E32 * dsa.sum(0))
        self.ds = ds

    def bound(self, name):
        a, b, mag = self.bounds[name]
        return a * getattr(self, name).abs() + b * mag + FLOOR * (float(mag.max()) if mag.numel() else 0.0)

    def ratio(self, name, mine):
        """worst |mine - ref| / bound over every element (inf for a NaN or a miss of a zero bound)"""
        want = getattr(self, name)
        mine = mine.double().reshape(want.shape)
        err, bound = (mine - want).abs(), self.bound(name)
        r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float('inf'), 0.0))
        return float(torch.nan_to_num(r, nan=float('inf')).max()) if r.numel() else 0.0

    def check(self, results, record=None, scale=1.0):
        """results: {name: tensor in the unit layout}; every element of every tensor is compared.  -> {name: worst |err| / bound};
        raises AssertionError past `scale`."""
        worst = {name: self.ratio(name, t) for name, t in results.items() if t is not None}
        if record is not None:
            record(worst)
        bad = {k: v for k, v in worst.items() if not v <= scale}
        assert not bad, f'|err| / bound past {scale}: {bad} (all: {worst})'
        return worst


def autograd(q, k, v, dout, bias=None, qimg=None):
    """plain softmax(Q K^T s + bias) V and torch's own backward in fp64 -> out, lse, dq (of q as given), dk, dv, dbias"""
    D = k.shape[-1]
    q, k, v = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    b = None if bias is None else bias.double().clone().requires_grad_(True)
    qu = q if qimg is None else q[qimg]
    s = (qu @ k.transpose(-2, -1)) * SCALE[D]
    if b is not None:
        s = s + b
    o = torch.softmax(s, -1) @ v
    o.backward(dout.double())
    return o.detach(), torch.logsumexp(s.detach(), -1), q.grad, k.grad, v.grad, None if b is None else b.grad


def emulate(q, k, v, dout, bias=None, qimg=None, family='dense', variant=None):
    """The kernels' rounding points in fp32 (not their summation order): P to bf16 before P V and before dV, O to bf16 (and, dense,
    into delta), dS to bf16 before dQ / dK and fp32 into dbias, results to bf16.  -> the dict Ref.check takes.
    variant: a defect the bounds must catch: 'extra_key' (a zero key past N joins the softmax), 'no_alpha' (the row sum of every
    tile but the last is counted 2x), 'scale32' (32^-0.5 at head_dim 64 and the reverse), 'dbias_bf16' (dS rounded in dbias)."""
    BF = torch.bfloat16
    U, H, N, D = k.shape
    sc = SCALE[D] if variant != 'scale32' else SCALE[96 - D]
    q, k, v, go = q.float(), k.float(), v.float(), dout.float()
    qu = q if qimg is None else q[qimg]
    s = (qu @ k.transpose(-2, -1)) * sc
    if bias is not None:
        s = s + bias.float()
    m = s.amax(-1, keepdim=True)
    if variant == 'extra_key':
        m = m.clamp_min(0.0)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    if variant == 'extra_key':
        l = l + torch.exp(-m)
    if variant == 'no_alpha' and N > TL:
        l = l + e[..., :(N - 1) // TL * TL].sum(-1, keepdim=True)
    lse = (m + torch.log(l)).squeeze(-1)
    o = (e.to(BF).float() @ v) / l
    ob = o.to(BF)
    p = torch.exp(s - lse.unsqueeze(-1))
    dp = go @ v.transpose(-2, -1)
    delta = (go * ob.float()).sum(-1, keepdim=True) if family == 'dense' else (p * dp).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    dsb = ds.to(BF).float()
    dq, dk, dv = (dsb @ k) * sc, (dsb.transpose(-2, -1) @ qu) * sc, p.to(BF).float().transpose(-2, -1) @ go
    res = {'out': ob, 'lse': lse, 'dk': dk.to(BF), 'dv': dv.to(BF)}
    if qimg is None:
        res['dq'] = dq.to(BF)
    else:
        res['dq_global'] = torch.zeros_like(q).index_add_(0, qimg, dq).to(BF)
    if bias is not None:
        res['dbias'] = (dsb if variant == 'dbias_bf16' else ds).sum(0)
    return res


# ---- input makers ----------------------------------------------------------------------------------------------------------------
KINDS = ('random', 'max_last', 'max_first', 'alternate', 'bias_decides', 'tile_masked', 'first_tile_masked', 'row_masked', 'uniform',
         'dout_zero', 'dout_one_row')
MASK = -3.0e4


def alternate_key(n):
    """the key row i of 'alternate' puts its maximum on: tile i mod nt, so consecutive rows peak in different key tiles"""
    i = torch.arange(n)
    t = i % cdiv(n, TL)
    return t * TL + (i * 7) % (n - t * TL).clamp_max(TL)


def decided_key(n):
    """the key the bias of 'bias_decides' moves row i's maximum to"""
    return (torch.arange(n) * 5 + 3) % n


def masked_rows(n):
    """the query rows whose tile 'tile_masked' / 'first_tile_masked' masks: every third"""
    return torch.arange(n) % 3 == 0


def masked_tile(n, first):
    """keys [lo, hi) of the masked tile: the first tile, or the last full one that is not the first"""
    if first:
        return 0, min(TL, n)
    t = max((n // TL) - 1, 1) if n > TL else 0
    return t * TL, min((t + 1) * TL, n)


def make(kind, units, heads, n, hd, seed, biased, uq=None):
    """bf16 q [uq or units][heads][n][hd], k, v, dout [units][heads][n][hd] and an fp32 bias [heads][n][n] (None unless `biased`).
      random             N(0, 1.5^2) operands, bias N(0, 2^2)
      max_last           every row's maximum on key n - 1, >= 100 nats above the rest (rows one-hot)
      max_first          on key 0, every other key >= 100 nats below
      alternate          row i peaks on alternate_key(i), 8 nats up: the running maximum moves by a few nats from tile to tile
      bias_decides       Q K^T puts 20 ... 35 nats on key 0, a bias of +100 on decided_key(i) wins (needs `biased`)
      tile_masked        `random` with a bias of -3e4 on one whole key tile (not the first) for masked_rows (needs `biased`)
      first_tile_masked  the same on the first tile
      row_masked         `random` with -3e4 added to EVERY key of masked_rows: the softmax is the same, lse is about -3e4, and
                         exp2(-lse log2e) overflows: a key past N that is not masked out of dS turns dQ into NaN (needs `biased`)
      uniform            q = 0 and bias = 0: every row uniform
      dout_zero          `random` with dout = 0
      dout_one_row       `random` with dout nonzero in token n // 2 of unit 0, head heads - 1 only"""
    assert kind in KINDS
    g = torch.Generator().manual_seed(seed)
    uq = units if uq is None else uq
    q = torch.randn(uq, heads, n, hd, generator=g) * 1.5
    k = torch.randn(units, heads, n, hd, generator=g) * 1.5
    v = torch.randn(units, heads, n, hd, generator=g) * 1.5
    dout = torch.randn(units, heads, n, hd, generator=g)
    bias = torch.randn(heads, n, n, generator=g) * 2 if biased else None
    sc = SCALE[hd]
    sign = torch.where(torch.rand(hd, generator=g) < 0.5, -1.0, 1.0)
    if kind in ('max_last', 'max_first', 'bias_decides'):
        amp = ((30.0 if kind == 'bias_decides' else 130.0) / (sc * hd)) ** 0.5      # 30 or 130 nats on the chosen key
        key = n - 1 if kind == 'max_last' else 0
        q = q * (0.5 / 1.5) + amp * sign
        k = k * (0.1 / 1.5)
        k[:, :, key] = amp * sign
        if bias is not None:
            bias = bias * 0.5
        if kind == 'bias_decides':
            assert biased
            bias[:, torch.arange(n), decided_key(n)] += 100.0
    elif kind == 'alternate':
        k = k / 1.5
        src = (k[torch.arange(uq) % units] if uq != units else k)[:, :, alternate_key(n)]
        q = src * (8.0 / (sc * (src * src).sum(-1, keepdim=True)))             # 8 nats on its own key, N(0, ~1.4^2) elsewhere
        if bias is not None:
            bias = bias * 0.1
    elif kind in ('tile_masked', 'first_tile_masked'):
        assert biased
        lo, hi = masked_tile(n, kind == 'first_tile_masked')
        rows = masked_rows(n)
        bias[:, rows, lo:hi] = MASK
    elif kind == 'row_masked':
        assert biased
        bias[:, masked_rows(n)] += MASK
    elif kind == 'uniform':
        q = torch.zeros_like(q)
        bias = None if bias is None else torch.zeros_like(bias)
    elif kind == 'dout_zero':
        dout = torch.zeros_like(dout)
    elif kind == 'dout_one_row':
        keep = dout[0, heads - 1, n // 2].clone()
        dout = torch.zeros_like(dout)
        dout[0, heads - 1, n // 2] = keep
    BF = torch.bfloat16
    return q.to(BF), k.to(BF), v.to(BF), dout.to(BF), bias
