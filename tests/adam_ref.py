"""CPU restatement of the Adam update kernel (csrc/train_step.hip: adam_scalars_kernel, adam_kernel behind snerf_adam_step_f32),
used ONLY by tests.  The kernel documents its statements (train_step.hip, "Adam"):

    grad        = fma(weight_decay, param, grad)                      (only if weight_decay != 0)
    exp_avg     = fma(1 - beta1, grad - exp_avg, exp_avg)
    exp_avg_sq  = fma((1 - beta2) * grad, grad, exp_avg_sq * beta2)
    denom       = sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps
    param       = param + (-(lr / (1 - beta1^t)) * exp_avg) / denom

in fp32, every operation rounded once, with t = step[0] + 1 of the element's range.  Here they are restated so that NO rounding is
left to chance:

  * f32_add / sub / mul / div / sqrt: fp32 operands, the operation in float64, one rounding to fp32.  Correct (no double rounding)
    because float64 carries 53 >= 2 * 24 + 2 bits;
  * fma32(): that argument does not hold for a * b + c (the exact sum can need hundreds of bits).  The product of two fp32 numbers
    is exact in float64; the sum with c is split into its float64 rounding and the exact error (TwoSum), the float64 sum is moved to
    the neighbour with an odd last bit when it is inexact (round to odd), and that rounds to fp32 like the exact sum would.
    tests/test_adam_host.py holds it to rational arithmetic, subnormal results included;
  * scalars(): -(lr / (1 - beta1^t)) and sqrt(1 - beta2^t) from 120-digit decimal arithmetic on the doubles the caller passes,
    rounded once to fp32 (round_fraction_f32).  The kernel gets there through a float64 pow / divide / sqrt and a conversion, so it
    can differ only where the exact value lies within a few float64 ulps of an fp32 rounding boundary: scalar_headroom() measures the
    relative distance to the nearest fp32 midpoint and the host test requires 2^-40 for every (lr, beta1, beta2, t) a case uses;
  * the constants 1 - beta1, beta2, 1 - beta2, eps, weight_decay: computed in float64 and converted to fp32, as the entry does;
  * nothing is flushed: subnormal moments keep their bits.  NaN (eps = 0 with a zero gradient: 0 / 0) is compared by position.

Also here: the cases of tests/test_gpu_adam.py as named records (CASES), their inputs, the run of a case step by step (run()), and
VARIANTS - the restatement made wrong on purpose, one statement at a time - with which tests/test_adam_host.py shows that a bit-for-bit
comparison on these cases tells each of them from the kernel's statements.
"""
import decimal
import functools
import math
import os
from collections import namedtuple
from fractions import Fraction

import numpy as np

F32 = np.float32
F64 = np.float64
MAX_RANGES, MAX_NETS = 32, 8          # csrc/train_step.hip: ADAM_MAX_RANGES, ADAM_MAX_NETS
HEADROOM = 2.0 ** -40                 # required relative distance of an exact scalar from the nearest fp32 midpoint
_CTX = decimal.Context(prec=120, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)


# ------------------------------------------------------------------------------------------------ fp32 operations, rounded once
def _f64(x):
    x = np.asarray(x)
    assert x.dtype == F32, x.dtype
    return x.astype(F64)


def _binary(op, a, b):
    with np.errstate(all="ignore"):
        return op(_f64(a), _f64(b)).astype(F32)


def f32_add(a, b):
    return _binary(np.add, a, b)


def f32_sub(a, b):
    return _binary(np.subtract, a, b)


def f32_mul(a, b):
    return _binary(np.multiply, a, b)


def f32_div(a, b):
    return _binary(np.divide, a, b)


def f32_sqrt(a):
    with np.errstate(all="ignore"):
        return np.sqrt(_f64(a)).astype(F32)


def fma32(a, b, c):
    """round_to_fp32(a * b + c) with the product and the sum exact (module docstring)."""
    a, b, c = _f64(a), _f64(b), _f64(c)
    with np.errstate(all="ignore"):
        p = a * b                                   # 24 x 24 bits: exact
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)                 # TwoSum: s + e == p + c exactly
        inexact = np.isfinite(s) & (e != 0)
        even = (s.view(np.int64) & 1) == 0
        odd = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))      # the exact sum lies between s and this neighbour
        return np.where(inexact & even, odd, s).astype(F32)


def fma32_naive(a, b, c):
    """what fma32 must NOT be: the float64 sum rounded to nearest, then to fp32 (two roundings)"""
    with np.errstate(all="ignore"):
        return (_f64(a) * _f64(b) + _f64(c)).astype(F32)


def round_fraction_f32(x):
    """a rational number to the nearest fp32, ties to even, subnormals and overflow as IEEE 754 has them"""
    x = Fraction(x)
    if x == 0:
        return F32(0.0)
    sign, x = (-1.0 if x < 0 else 1.0), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1                                     # 2^e <= x < 2^(e + 1)
    q = max(e, -126) - 23                          # exponent of the last place
    n = round(x / Fraction(2) ** q)                # Python rounds a Fraction half to even
    if n * Fraction(2) ** q >= Fraction(2) ** 128:
        return F32(sign * math.inf)
    return F32(sign * math.ldexp(n, q))


def fma_fraction(a, b, c):
    """the same through rational arithmetic, one element (finite operands)"""
    return round_fraction_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


# ------------------------------------------------------------------------------------------------ the step-dependent scalars
def _exact_scalars(lr, beta1, beta2, t):
    """(-(lr / (1 - beta1^t)), sqrt(1 - beta2^t)) as 120-digit decimals of the doubles lr, beta1, beta2"""
    d = lambda v: _CTX.create_decimal(float(v))       # a double converts exactly
    bc1 = _CTX.subtract(1, _CTX.power(d(beta1), t))
    bc2 = _CTX.subtract(1, _CTX.power(d(beta2), t))
    return _CTX.minus(_CTX.divide(d(lr), bc1)), _CTX.sqrt(bc2)


def scalar_headroom(x):
    """relative distance of the exact value x (Decimal) from the nearest fp32 midpoint; inf for 0 (which fp32 holds)"""
    x = Fraction(x)
    if x == 0:
        return math.inf
    f = round_fraction_f32(x)
    mids = [(Fraction(float(f)) + Fraction(float(np.nextafter(f, F32(side))))) / 2 for side in (-np.inf, np.inf)
            if np.isfinite(np.nextafter(f, F32(side)))]
    return float(min(abs(x - m) for m in mids) / abs(x))


@functools.lru_cache(maxsize=None)
def scalars(lr, beta1, beta2, t):
    """(neg_step, bc2_sqrt) as fp32 and their headrooms, for t >= 1"""
    assert t >= 1
    a, b = _exact_scalars(lr, beta1, beta2, t)
    neg = F32(-0.0) if a == 0 else round_fraction_f32(Fraction(a))       # lr = 0: -(0 / bc1) is -0
    return neg, round_fraction_f32(Fraction(b)), scalar_headroom(a), scalar_headroom(b)


def scalars_f32_pow(lr, beta1, beta2, t):
    """VARIANT: the bias corrections in fp32 - beta rounded to fp32, a correctly rounded fp32 pow (no libm: the same on every host),
    fp32 subtraction, division and root"""
    def pow32(beta):
        return round_fraction_f32(Fraction(_CTX.power(_CTX.create_decimal(float(F32(beta))), t))) if t > 0 else F32(1.0)
    with np.errstate(all="ignore"):
        one = F32(1.0)
        return F32(-(F32(lr) / (one - pow32(beta1)))), F32(np.sqrt(one - pow32(beta2)))


def scalars_at(lr, beta1, beta2, t):
    """scalars() for any t >= 0 in float64 semantics (t = 0 only arises in a VARIANT: 1 - beta^0 = 0)"""
    if t == 0:
        with np.errstate(all="ignore"):
            return F32(-(F64(lr) / F64(0.0))), F32(0.0)
    return scalars(lr, beta1, beta2, t)[:2]


# ------------------------------------------------------------------------------------------------ one update
Hyper = namedtuple("Hyper", "lr beta1 beta2 eps wd")
DEFAULT = Hyper(3e-3, 0.9, 0.999, 1e-8, 0.0)

# the restatement made wrong, one statement at a time (what a bit-for-bit comparison has to tell from the kernel's statements)
VARIANTS = ("wd_unfused", "lerp_unfused", "sq_unfused", "sqrt_of_quotient", "eps_inside_root", "wd_after_moments",
            "neighbour_scalars", "t_not_t_plus_1", "f32_pow")


def constants(h):
    """the fp32 constants the entry hands to the kernel: w1, beta2, w2, eps, wd"""
    return F32(1.0 - h.beta1), F32(h.beta2), F32(1.0 - h.beta2), F32(h.eps), F32(h.wd)


def update(p, g, m, v, neg_step, bc2_sqrt, h, variant=None):
    """the five statements on fp32 arrays (neg_step, bc2_sqrt: per element); returns the new (p, m, v)"""
    w1, beta2, w2, eps, wd = constants(h)
    full = lambda s: np.full(p.shape, s, F32)
    decayed = g
    if wd != 0:
        decayed = f32_add(f32_mul(full(wd), p), g) if variant == "wd_unfused" else fma32(full(wd), p, g)
    if variant != "wd_after_moments":
        g = decayed
    d = f32_sub(g, m)
    m = f32_add(f32_mul(full(w1), d), m) if variant == "lerp_unfused" else fma32(full(w1), d, m)
    w2g, vb = f32_mul(full(w2), g), f32_mul(v, full(beta2))
    v = f32_add(f32_mul(w2g, g), vb) if variant == "sq_unfused" else fma32(w2g, g, vb)
    if variant == "sqrt_of_quotient":
        denom = f32_add(f32_sqrt(f32_div(v, f32_mul(bc2_sqrt, bc2_sqrt))), full(eps))
    elif variant == "eps_inside_root":
        denom = f32_div(f32_sqrt(f32_add(v, full(eps))), bc2_sqrt)
    else:
        denom = f32_add(f32_div(f32_sqrt(v), bc2_sqrt), full(eps))
    if variant == "wd_after_moments" and wd != 0:      # the decay applied to the parameter instead (decoupled, AdamW's order)
        p = fma32(f32_mul(full(-F32(h.lr)), full(wd)), p, p)
    p = f32_add(p, f32_div(f32_mul(neg_step, m), denom))
    return p, m, v


# ------------------------------------------------------------------------------------------------ the cases
# ranges: (begin, end, n_steps, preset) - parameters [begin, end) with n_steps device counters, all holding `preset` before the first
# step.  skips: {iteration: ranges left out of that call}.  grads: the generator of gradients() below.  init: "normal" - parameters
# ~ N(0, 0.5), some of them within a few steps of zero, which they cross - or "away_from_zero", 0.25 <= |p| < 1, for the cases that are
# also held against torch.optim.Adam: torch's sqrt may round the other way, its update then differs by one unit in ITS last place
# (lr 3e-3: at most 2^-32), and that shows as at most one unit in the last place of a parameter only while the parameter is not much
# smaller than the update (a parameter that cancels to 1e-4 shows the same 2e-10 as 32 units: cancellation, not another update).
Range = namedtuple("Range", "begin end n_steps preset")
Case = namedtuple("Case", "name n ranges hyper iters skips grads init seed")


def make_case(name, n, ranges, hyper=DEFAULT, iters=3, skips=None, grads="plain", init="normal", seed=1):
    ranges = tuple(Range(*r) for r in ranges)
    assert len(ranges) <= MAX_RANGES
    for a, b in zip(ranges, ranges[1:]):
        assert a.end <= b.begin
    assert all(0 <= r.begin <= r.end <= n and r.n_steps >= 1 and r.preset >= 0 for r in ranges)
    return Case(name, n, ranges, hyper, iters, dict(skips or {}), grads, init, seed)


def _many_ranges():
    out, at = [], 2
    for r in range(MAX_RANGES):
        size = 1 + (53 * r) % 131
        out.append((at, at + size, (1, 64, 65, 130)[r % 4], (37 * r * r + 11 * r) % 5000))
        at += size + r % 3                         # 0, 1 or 2 parameters between two ranges belong to none
    return at + 5, out


_MANY_N, _MANY = _many_ranges()
_TWO = [(0, 700, 3, 0), (700, 2000, 2, 3)]
CASES = [
    make_case("defaults", 2000, _TWO, iters=6, grads="wide", init="away_from_zero"),
    make_case("defaults_wd", 2000, _TWO, DEFAULT._replace(wd=0.01), iters=6, grads="wide", init="away_from_zero"),
    make_case("boundaries", 1600, [(0, 1, 1, 0), (1, 257, 2, 5), (257, 257, 1, 17), (257, 1000, 3, 999), (1003, 1500, 1, 100000)]),
    make_case("many_ranges", _MANY_N, _MANY, Hyper(1e-3, 0.9, 0.999, 1e-8, 1e-4)),
    make_case("tiny_and_huge", 3000, [(0, 1300, 1, 0), (1300, 3000, 4, 0)], iters=6, grads="tiny_and_huge", init="away_from_zero"),
    make_case("eps0", 700, [(3, 300, 1, 0), (300, 690, 2, 2)], DEFAULT._replace(eps=0.0), iters=4, grads="zeros_first"),
    make_case("lr0", 600, [(0, 290, 1, 0), (290, 600, 1, 7)], DEFAULT._replace(lr=0.0, wd=0.01)),
    make_case("beta1_0", 600, [(0, 290, 1, 0), (290, 600, 1, 7)], DEFAULT._replace(beta1=0.0)),
    make_case("beta2_0", 600, [(0, 290, 1, 0), (290, 600, 1, 7)], DEFAULT._replace(beta2=0.0)),
    make_case("betas_near_1", 600, [(0, 290, 1, 0), (290, 600, 1, 40)], DEFAULT._replace(beta1=0.99, beta2=0.9999), iters=4),
    make_case("skipped", 900, [(0, 300, 2, 0), (300, 613, 3, 0), (613, 900, 1, 0)], iters=5, skips={1: (1,), 2: (1,)}),
]
CASE = {c.name: c for c in CASES}
TORCH_CASES = ("defaults", "defaults_wd", "tiny_and_huge")      # held against torch.optim.Adam on the CPU as well


def _rng(case, *more):
    return np.random.default_rng([case.seed, case.n, len(case.ranges), *more])


def initial_params(case):
    rng = _rng(case, 0)
    if case.init == "away_from_zero":
        return (rng.choice(np.array([-1.0, 1.0]), case.n) * rng.uniform(0.25, 1.0, case.n)).astype(F32)
    return rng.normal(0.0, 0.5, case.n).astype(F32)


def gradients(case, k):
    """the fp32 gradient of every element of the buffer for iteration k (elements outside the call's ranges are never read)"""
    rng, n = _rng(case, 1, k), case.n
    sign = rng.choice(np.array([-1.0, 1.0]), n)
    if case.grads == "plain":                          # what training sees: 1e-4 .. 1
        g = rng.normal(size=n) * 10.0 ** rng.uniform(-4.0, 0.0, n)
    else:                                              # per-element magnitudes that stay put over the steps
        hi = 15.0 if case.grads == "tiny_and_huge" else 0.0
        mag = 10.0 ** _rng(case, 2).uniform(-30.0, hi, n)
        g = sign * mag * rng.uniform(0.5, 1.5, n)
        zero = _rng(case, 3).uniform(size=n)
        if case.grads == "zeros_first":
            g[(zero < 0.3) & (k == 0)] = 0.0           # 0 / 0 with eps = 0 ...
            g[zero < 0.1] = 0.0                        # ... on every step for some
        else:
            g[(zero < 0.1) & (k in (2, 3))] = 0.0      # exactly 0 after non-zero steps
            g[zero > 0.97] = 0.0                       # never a gradient: both moments stay 0
    return g.astype(F32)


def active_ranges(case, k):
    skipped = case.skips.get(k, ())
    return [i for i in range(len(case.ranges)) if i not in skipped]


Run = namedtuple("Run", "params exp_avg exp_avg_sq steps scal")


@functools.lru_cache(maxsize=None)
def _run_cached(case_key, variant):
    return _run(CASE[case_key], variant)


def run(case, variant=None):
    """The state after every call: params / exp_avg / exp_avg_sq [iters + 1, n] (row 0: before the first call), steps [iters + 1,
    ranges] (the value all counters of a range hold) and scal[k] = {range: (neg_step, bc2_sqrt)} of call k.  Read-only, shared."""
    if CASE.get(case.name) is case:
        return _run_cached(case.name, variant)
    return _run(case, variant)


def _run(case, variant):
    assert variant is None or variant in VARIANTS
    h, n = case.hyper, case.n
    p, m, v = initial_params(case), np.zeros(n, F32), np.zeros(n, F32)
    t = [r.preset for r in case.ranges]
    P, M, V, T, S = [p], [m], [v], [list(t)], []
    for k in range(case.iters):
        g = gradients(case, k)
        act = active_ranges(case, k)
        sc = {}
        for i in act:
            t[i] += 1
            tt = t[i] - 1 if variant == "t_not_t_plus_1" else t[i]
            sc[i] = scalars_f32_pow(h.lr, h.beta1, h.beta2, tt) if variant == "f32_pow" else scalars_at(h.lr, h.beta1, h.beta2, tt)
        neg, bc2 = np.zeros(n, F32), np.ones(n, F32)
        on = np.zeros(n, bool)
        for j, i in enumerate(act):
            r = case.ranges[i]
            on[r.begin:r.end] = True
            neg[r.begin:r.end], bc2[r.begin:r.end] = sc[i]
            if variant == "neighbour_scalars" and r.end > r.begin:
                if j > 0:
                    neg[r.begin], bc2[r.begin] = sc[act[j - 1]]
                if j + 1 < len(act):
                    neg[r.end - 1], bc2[r.end - 1] = sc[act[j + 1]]
        gp = np.where(on, g, F32(0.0))
        pn, mn, vn = update(p, gp, m, v, neg, bc2, h, variant)
        p, m, v = (np.where(on, a, b) for a, b in ((pn, p), (mn, m), (vn, v)))
        P.append(p), M.append(m), V.append(v), T.append(list(t)), S.append(sc)
    out = Run(np.stack(P), np.stack(M), np.stack(V), np.array(T, np.int64).reshape(case.iters + 1, len(case.ranges)), S)
    for a in out[:4]:
        a.setflags(write=False)
    return out


def case_scalar_inputs(case):
    """every (lr, beta1, beta2, t) the case's calls use"""
    h, t, out = case.hyper, [r.preset for r in case.ranges], []
    for k in range(case.iters):
        for i in active_ranges(case, k):
            t[i] += 1
            out.append((h.lr, h.beta1, h.beta2, t[i]))
    return sorted(set(out))


# ------------------------------------------------------------------------------------------------ comparison
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F32 else a


def differing(got, want):
    """indices at which two arrays differ: NaN by position, every other value (signed zeros, subnormals) by its bits"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype != F32:
        return np.flatnonzero(got != want)
    gn, wn = np.isnan(got), np.isnan(want)
    return np.flatnonzero((gn != wn) | (~wn & (bits(got) != bits(want))))


def range_of(case, i):
    for k, r in enumerate(case.ranges):
        if r.begin <= i < r.end:
            return f"range {k} [{r.begin}, {r.end})"
    return "no range"


def assert_same_bits(case, what, got, want):
    bad = differing(got, want)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{case.name}: {what}: {bad.size} of {want.size} elements differ, first at {i} ({range_of(case, i)}): "
                             f"got {got[i]!r} (0x{int(bits(got)[i]):08x}), want {want[i]!r} (0x{int(bits(want)[i]):08x})")


def variant_changes(case, variant):
    """number of elements of the final (params, exp_avg, exp_avg_sq) the variant changes"""
    a, b = run(case), run(case, variant)
    return sum(int(differing(x[-1], y[-1]).size) for x, y in zip(a[:3], b[:3]))


def describe(case):
    """one line for profiles/adam_exact_cases.txt"""
    h = case.hyper
    rs = " ".join(f"[{r.begin},{r.end})x{r.n_steps}@{r.preset}" for r in case.ranges)
    skips = "".join(f" skip{k}:{list(v)}" for k, v in sorted(case.skips.items()))
    return (f"{case.name:<14} n {case.n:<5} steps {case.iters} lr {h.lr:g} betas ({h.beta1:g}, {h.beta2:g}) eps {h.eps:g} wd {h.wd:g} "
            f"grads {case.grads} params {case.init}{skips}\n    {len(case.ranges)} ranges [begin,end)xcounters@preset: {rs}")


# ------------------------------------------------------------------------------------------------ torch.optim.Adam on the CPU
def ulp_distance(a, b):
    """how many fp32 values apart (finite arrays)"""
    def ordered(x):
        i = bits(x).astype(np.int64)
        return np.where(i < 2 ** 31, i, 2 ** 31 - i)
    return np.abs(ordered(a) - ordered(b))


def torch_comparison(case):
    """The case through torch.optim.Adam on the CPU - one tensor per range, the same gradients, a range that a call leaves out having
    no .grad - against run(case) after the last call.  Returns the counters of both sides, the number of moment entries that differ,
    the largest distance of two parameters in units in the last place and how many parameters differ at all."""
    import torch
    h, ref = case.hyper, run(case)
    p0 = initial_params(case)
    params = [torch.nn.Parameter(torch.from_numpy(p0[r.begin:r.end].copy())) for r in case.ranges]
    opt = torch.optim.Adam(params, lr=h.lr, betas=(h.beta1, h.beta2), eps=h.eps, weight_decay=h.wd, foreach=False)
    for q, r in zip(params, case.ranges):
        opt.state[q] = {"step": torch.tensor(float(r.preset)), "exp_avg": torch.zeros_like(q), "exp_avg_sq": torch.zeros_like(q)}
    for k in range(case.iters):
        g, act = gradients(case, k), active_ranges(case, k)
        for i, (q, r) in enumerate(zip(params, case.ranges)):
            q.grad = torch.from_numpy(g[r.begin:r.end].copy()) if i in act else None
        opt.step()
    cat = lambda key: np.concatenate([opt.state[q][key].numpy() for q in params])
    covered = np.concatenate([np.arange(r.begin, r.end) for r in case.ranges])
    got_p = np.concatenate([q.detach().numpy() for q in params])
    want_p = ref.params[-1][covered]
    dist = ulp_distance(got_p, want_p)
    return {"steps_torch": [int(opt.state[q]["step"]) for q in params], "steps_ref": [int(t) for t in ref.steps[-1]],
            "exp_avg_diff": int(differing(cat("exp_avg"), ref.exp_avg[-1][covered]).size),
            "exp_avg_sq_diff": int(differing(cat("exp_avg_sq"), ref.exp_avg_sq[-1][covered]).size),
            "max_ulp": int(dist.max()), "params_diff": int((dist != 0).sum()), "n": int(covered.size)}


# ------------------------------------------------------------------------------------------------ the record
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "adam_exact_cases.txt")
TORCH_TAG = "torch.optim.Adam "      # lines that depend on the host's torch build (its vectorised sqrt)


def variant_table():
    """{variant: {case name: changed elements}}"""
    return {v: {c.name: variant_changes(c, v) for c in CASES} for v in VARIANTS}


def profile_text():
    """the part of profiles/adam_exact_cases.txt that is the same on every host"""
    out = ["# tests/adam_ref.py: the cases of tests/test_gpu_adam.py (rewrite with `python tests/adam_ref.py`; tests/test_adam_host.py compares).",
           "# headroom: the smallest relative distance of an exact -(lr / (1 - beta1^t)) or sqrt(1 - beta2^t) of the case from an fp32",
           "# rounding boundary, as a power of two (required: 2^-40); after it what the final state holds.", ""]
    for c in CASES:
        r = run(c)
        head = min(min(scalars(*k)[2:]) for k in case_scalar_inputs(c))
        ts = sorted({k[3] for k in case_scalar_inputs(c)})
        v, tiny = r.exp_avg_sq[1:], float(np.finfo(F32).tiny)
        out += [describe(c), f"    t of the calls: {ts[:12]}{' ...' if len(ts) > 12 else ''} ({len(ts)} values)   headroom 2^{math.log2(head):.1f}",
                f"    exp_avg_sq over the steps: {int((v == 0).sum())} zero, {int(((v != 0) & (v < tiny)).sum())} subnormal, largest {float(v.max()):.3g};"
                f" NaN parameters at the end: {int(np.isnan(r.params[-1]).sum())}", ""]
    table = variant_table()
    out += ["# elements of the final (params, exp_avg, exp_avg_sq) that each wrong variant of the restatement changes, case by case",
            "# " + " ".join(f"{i}={c.name}" for i, c in enumerate(CASES)),
            f"{'variant':<18}" + "".join(f"{i:>6}" for i in range(len(CASES))) + "   cases"]
    for v in VARIANTS:
        out.append(f"{v:<18}" + "".join(f"{table[v][c.name]:>6}" for c in CASES) + f"   {sum(1 for c in CASES if table[v][c.name])}")
    return "\n".join(out) + "\n"


def torch_lines():
    out = ["# against torch.optim.Adam on the CPU of the host that wrote this file (tests/test_adam_host.py caps a run at 4 x the larger of these",
           "# counts and of what the known share of misrounded roots predicts: torch's vectorised sqrt differs from host to host; wd = 0: exact moments)"]
    for name in TORCH_CASES:
        m = torch_comparison(CASE[name])
        out.append(f"{TORCH_TAG}{name}: parameters that differ {m['params_diff']} of {m['n']} (largest distance {m['max_ulp']} ulp), "
                   f"exp_avg {m['exp_avg_diff']}, exp_avg_sq {m['exp_avg_sq_diff']}")
    return "\n".join(out) + "\n"


def recorded_torch_counts(text):
    """{case name: parameters that differed on the host that wrote the profile}"""
    out = {}
    for line in text.splitlines():
        if line.startswith(TORCH_TAG):
            name, rest = line[len(TORCH_TAG):].split(":", 1)
            out[name] = int(rest.split("differ", 1)[1].split()[0])
    return out


def stable_part(text):
    return "".join(l + "\n" for l in text.splitlines() if not l.startswith(TORCH_TAG) and not l.startswith("# against torch") and
                   not l.startswith("# counts and of what"))


if __name__ == "__main__":
    with open(PROFILE, "w") as f:
        f.write(profile_text() + "\n" + torch_lines())
    print("wrote", PROFILE)
