"""fp64 one-step formulas of the flat-arena optimizers as csrc/optim.hip states them, with the bound of every array the step
writes.  tests/test_optim_ref.py ties the formulas to torch.optim.SGD / Adam / AdamW / RMSprop run in float64 (1e-12 over six
steps, every configuration below); tests/test_optim_contract_gpu.py holds the device to them, one step at a time from the device's
own previous state, so that a bound stays a one-step bound.

Hyper-parameters cross the C ABI as floats.  The device tests hand these formulas the float values the kernel received
(`f32`), not the decimal literals: 1 - beta2 of float(0.999) is 0.99998713e-3, 1.3e-5 away from 1e-3, and that difference
belongs to the ABI, not to the kernel's arithmetic.

Bounds.  Every function returns (new, bound): `new` the arrays in fp64, `bound` for each array the number that, multiplied by
U32 = 2^-24, bounds |device - new| element by element.  A bound is `b * mag`: mag the same update on absolute values with
every subtraction turned into an addition, b the count of fp32 roundings on the longest path from the inputs to the stored
value (an addition of two terms with k1 and k2 roundings behind them has max(k1, k2) + 1: each term's error is relative to
its own magnitude).  Contraction to FMA only removes roundings.  sqrtf and the fp32 division are allowed 2 ulp each (HIP does not
promise correct rounding).  Counted from the kernel source (the functions use the count of the path a configuration
really takes — d is exact without weight decay, the first momentum buffer is d itself — and the table gives the longest):

  d (the effective gradient)          SGD / Adam: g + wd * w, 2 roundings (0 without weight decay); RMSprop: fmaf(wd, w, g), 1.
  SGD      buf  = momentum * buf + (1 - dampening) * d      d (2), 1 - dampening (1), product (1), sum (1):            B_BUF = 5
           w    = w - lr * (d + momentum * buf')            buf' (5), product (1), sum (1), lr product (1), difference: B_SGD = 9
  Adam     m    = m + (d - m) * (1 - beta1)                 d (2), difference (1), 1 - beta1 (1), product (1), sum (1):  B_M = 6
           v    = beta2 * v + (1 - beta2) * d * d           d * d carries d's error twice (4) and its own rounding (1),
                                                            1 - beta2 (1), product (1), sum (1):                         B_V = 8
           denom = sqrtf(v) / bc2_sqrt + eps                v is a sum of non-negative terms once mag_v = v; in general its
                                                            relative error is B_V * kv, kv = mag_v / v >= 1.  The root halves it
                                                            (4 kv) and adds 2; bc2_sqrt is rounded once (1), the division 2, the
                                                            sum with eps >= 0 one more: E_DEN = 4 kv + 6 relative.
           w    = wdec - step_size * (m / denom)            the quotient: B_M mag_m / denom from m, (E_DEN + 2) |m| / denom from
                                                            denom and the division; step_size is rounded once and multiplied once
                                                            (2); wdec = w (1 - lr wd) has 3 roundings (AdamW), the difference 1:
                                                            bound_w = 4 (|w| + s |m| / denom) + s (B_M mag_m + (E_DEN + 4) |m|) / denom
                                                            — the form U32 (b1 |w| + b2 step_size mag_m / denom) with b1 = 4 and
                                                            b2 <= B_M + E_DEN + 8 = 4 kv + 20.
  RMSprop  sq   = alpha * sq + (1 - alpha) * d * d          d * d: 2 * 1 + 1, 1 - alpha (1), product (1), sum (1):        B_SQ = 6
           ga   = ga + (d - ga) * (1 - alpha)               d (1), difference, 1 - alpha, product, sum:                   B_GA = 5
           t    = sq - ga * ga  (centered)                  ga * ga: 2 * 5 + 1 = 11 on mag_ga^2; the difference 1:
                                                            relative error E_T = (B_SQ mag_sq + 11 mag_ga^2) / t + 1 — the
                                                            cancellation factor (sq + ga^2) / (sq - ga^2) in the open
                (plain)                                     E_T = B_SQ mag_sq / sq
           avg  = sqrtf(t) + eps                            E_AVG = E_T / 2 + 2 + 1
           q    = d / avg                                   (mag_d + (E_AVG + 2) |d|) / avg
           buf  = momentum * buf + q                        bound_q + momentum |buf| (the product) + mag_buf' (the sum)
           w    = w - lr * buf'  or  w - lr * q             lr bound + lr |.| (the product) + |w| + lr |.| (the difference)
The tests choose gradients for which (sq + ga^2) / (sq - ga^2) stays below 100 (`centered_factor`; asserted on these formulas by
tests/test_optim_ref.py), so that the centred bound stays a few hundred U32 of the update."""
import torch

F64 = torch.float64
B_BUF, B_SGD, B_M, B_V, B_SQ, B_GA = 5, 9, 6, 8, 6, 5

COUNTS = [1, 255, 257, 4096 * 256 + 17]         # the last: a second grid-stride trip (4096 blocks of 256 threads)
STEPS = 6

SGD_CONFIGS = {
    'plain': dict(lr=0.1, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False),
    'plain_wd': dict(lr=0.1, momentum=0.0, dampening=0.0, weight_decay=5e-4, nesterov=False, maximize=False),
    'momentum': dict(lr=0.1, momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=False, maximize=False),
    'dampening': dict(lr=0.1, momentum=0.9, dampening=0.1, weight_decay=1e-4, nesterov=False, maximize=True),
    'nesterov': dict(lr=0.1, momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=True, maximize=False),
}
ADAM_CONFIGS = {
    'adam': dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False, maximize=False, step0=1),
    'adam_wd': dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, decoupled=False, maximize=True, step0=1),
    'adamw': dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, decoupled=True, maximize=False, step0=1),
    'adamw_nowd': dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=True, maximize=False, step0=1),
    'adam_late': dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False, maximize=False, step0=100000),
}
RMSPROP_CONFIGS = {
    f'{"centered" if cen else "plain"}_m{mom}_wd{wd}': dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=wd, momentum=mom,
                                                            centered=cen, maximize=(cen and mom == 0.9 and wd == 0.0))
    for cen in (False, True) for mom in (0.0, 0.9) for wd in (0.0, 1e-4)}


def f32(v):
    """the value a C float argument carries"""
    return float(torch.tensor(v, dtype=torch.float32))


def as_f32(cfg):
    return {k: (f32(v) if isinstance(v, float) else v) for k, v in cfg.items()}


def problem(count, seed, steps=STEPS):
    """(w0 [count], gradients [steps][count]) in fp32: reals of unit scale, one gradient element in eight exactly zero (at
    positions that move from step to step), so that every element sees different gradients over the steps and the variance
    estimate of centred RMSprop stays away from zero"""
    g = torch.Generator().manual_seed(1000 + seed + 7 * count)
    w0 = torch.randn(count, generator=g)
    grads = torch.randn(steps, count, generator=g)
    grads[torch.rand(steps, count, generator=g) < 0.125] = 0.0
    return w0, grads


def _kappa(mag, val):
    """mag / val where val > 0, 1 where both vanish"""
    return torch.where(val > 0, mag / val.clamp_min(1e-300), torch.ones_like(val))


def _d(w, g, wd, maximize, roundings):
    d = -g if maximize else g
    if wd != 0:
        return d + wd * w, d.abs() + wd * w.abs(), roundings
    return d, d.abs(), 0


def sgd_step(w, g, buf, lr, momentum, dampening, weight_decay, nesterov, maximize, first):
    """-> ({'param', 'buf'}, bounds); buf may be None when momentum == 0.  The counts follow the path actually taken (no weight
    decay: d is exact; first step: buf = d), B_BUF and B_SGD are their largest values."""
    w, g = w.to(F64), g.to(F64)
    d, md, k = _d(w, g, weight_decay, maximize, 2)
    new, bound = {}, {}
    if momentum != 0:
        if first:
            b, mb, kb = d, md, k
        else:
            b = momentum * buf.to(F64) + (1 - dampening) * d
            mb = momentum * buf.to(F64).abs() + (1 - dampening) * md
            kb = k + 3                                  # 1 - dampening, the product, the sum
        new['buf'], bound['buf'] = b, kb * mb
        if nesterov:
            d, md, k = d + momentum * b, md + momentum * mb, kb + 2
        else:
            d, md, k = b, mb, kb
    new['param'] = w - lr * d
    bound['param'] = (k + 2) * (w.abs() + lr * md)      # the product with lr, the difference
    assert k + 2 <= B_SGD
    return new, bound


def adam_step(w, g, m, v, step, lr, beta1, beta2, eps, weight_decay, decoupled, maximize, **_):
    """step = the number of this step (>= 1) -> ({'param', 'm', 'v'}, bounds)"""
    w, g, m, v = w.to(F64), g.to(F64), m.to(F64), v.to(F64)
    kw = 0
    if weight_decay != 0 and decoupled:
        w, kw = w * (1 - lr * weight_decay), 3          # lr * wd, 1 - ., the product
        d, md, k = (-g if maximize else g), g.abs(), 0
    else:
        d, md, k = _d(w, g, weight_decay, maximize, 2)
    m1 = m + (d - m) * (1 - beta1)
    mm = m.abs() + (md + m.abs()) * (1 - beta1)
    v1 = beta2 * v + (1 - beta2) * d * d
    mv = beta2 * v + (1 - beta2) * md * md
    bm, bv = k + 4, 2 * k + 4
    assert bm <= B_M and bv <= B_V
    step_size = lr / (1 - beta1 ** step)
    denom = v1.sqrt() / (1 - beta2 ** step) ** 0.5 + eps
    e_den = bv / 2 * _kappa(mv, v1) + 6
    new = {'param': w - step_size * (m1 / denom), 'm': m1, 'v': v1}
    bound = {'m': bm * mm, 'v': bv * mv,
             'param': (kw + 1) * (w.abs() + step_size * m1.abs() / denom) + step_size * (bm * mm + (e_den + 4) * m1.abs()) / denom}
    return new, bound


def centered_factor(sq, ga):
    """(sq + ga^2) / (sq - ga^2) of centred RMSprop, 1 where both vanish"""
    return _kappa(sq + ga * ga, sq - ga * ga)


def rmsprop_step(w, g, sq, buf, ga, lr, alpha, eps, weight_decay, momentum, centered, maximize):
    """-> ({'param', 'sq', 'buf'?, 'ga'?}, bounds)"""
    w, g, sq = w.to(F64), g.to(F64), sq.to(F64)
    d, md, k = _d(w, g, weight_decay, maximize, 1)
    s1 = alpha * sq + (1 - alpha) * d * d
    ms = alpha * sq + (1 - alpha) * md * md
    bs, bg = 2 * k + 4, k + 4
    assert bs <= B_SQ and bg <= B_GA
    new, bound = {'sq': s1}, {'sq': bs * ms}
    if centered:
        ga = ga.to(F64)
        a1 = ga + (d - ga) * (1 - alpha)
        ma = ga.abs() + (md + ga.abs()) * (1 - alpha)
        new['ga'], bound['ga'] = a1, bg * ma
        t = s1 - a1 * a1
        e_t = _kappa(bs * ms + (2 * bg + 1) * ma * ma, t) + 1
    else:
        t = s1
        e_t = bs * _kappa(ms, s1)
    avg = t.sqrt() + eps
    e_avg = e_t / 2 + 3
    q = d / avg
    bq = (k * md + (e_avg + 2) * d.abs()) / avg
    if momentum > 0:
        b1 = momentum * buf.to(F64) + q
        mb = momentum * buf.to(F64).abs() + q.abs()
        bb = bq + momentum * buf.to(F64).abs() + mb
        new['buf'], bound['buf'] = b1, bb
        upd, bupd = b1, bb
    else:
        upd, bupd = q, bq
    new['param'] = w - lr * upd
    bound['param'] = lr * bupd + 2 * lr * upd.abs() + w.abs()
    return new, bound


def cases(configs, big):
    """(configuration name, count) pairs of one kernel: every configuration at the three small counts, `big` alone at the
    count past the grid cap"""
    return [(name, c) for name in configs for c in COUNTS[:3]] + [(big, COUNTS[3])]


SGD_CASES = cases(SGD_CONFIGS, 'nesterov')
ADAM_CASES = cases(ADAM_CONFIGS, 'adamw')
RMSPROP_CASES = cases(RMSPROP_CONFIGS, 'centered_m0.9_wd0.0001')
