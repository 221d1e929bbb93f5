"""The inline functions of csrc/peaq_wave.h -- what every kernel is made of -- one by one on the GPU
(peaq_debug_wave, include/peaq_amd.h) against plain high-precision references: mpmath for the functions, exact
rational arithmetic for the sums, on sweeps with fixed seeds AND on the structured edges where table forms, rounding
boundaries and lane permutations go wrong.  Every generated argument is compared; nothing is filtered out.

Error measure of a function: |got - exact| / ulp(round(exact)), the ulp of subnormal (and zero) results 2^-1074.

Where a bar comes from (BARS below):
  claim     peaq_wave.h states it against a correctly rounded operation: div_fast, sqrt_pos "<= 1 ulp";
  measured  peaq_wave.h's number was taken against OCML (itself good to ~1 ulp) or there is none: the worst error
            against the exact value over everything this file feeds the function, measured on an MI355X and recorded
            in DESIGN.md 4, + 0.5 ulp, rounded up to the next half (the margin is for arguments not drawn; the
            functions are deterministic);
  derived   pow: (e_log + 1/2) |y ln x| + e_exp ulp from the bars of its logarithm and exponential;
  counted   sums, scans, DFTs: K 2^-53 sum |terms| with K the roundings on a term's path, stated at each test.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

try:
    import mpmath
    mpmath.mp.prec = 160
except ImportError:                                   # pragma: no cover
    mpmath = None                                     # functions: long double instead (exact_pairs); scans and DFTs fail

pytestmark = pytest.mark.gpu

N_SWEEP = 1 << 16
U = 2.0 ** -53
TINY = 2.0 ** -1074

# function -> (worst error measured on the MI355X in ulp [None: the bar is a claim], bar in ulp = measured + 0.5,
# rounded up to the next half).  The table with the arguments of the worst cases: DESIGN.md 4.
# "log_tab@1" is log_tab / log_tab_nonneg on [1, 1 + 3/256): bins 0 and 1 of the table, where the result is at most as
# large as the terms it is formed from -- log1p(x - 1) alone in bin 0, ln C + log1p(r) with r < 0 in the lower half
# of bin 1 (peaq_wave.h: "<= 5 ulp" there, against OCML).  5.035 was met at 0x1.00ffe78d8148dp+0 by a sweep of 20 000
# arguments per bin made while this file was written (4.963 is the worst of the sweeps below); everything outside
# these two bins stayed below 1.98 in either.
BARS = {
    "log_pos": (1.894, 2.5), "log_nonneg": (1.894, 2.5), "log_tab": (1.974, 2.5), "log_tab_nonneg": (1.974, 2.5),
    "log_tab@1": (5.035, 6.0),
    "exp_fast": (2.285, 3.0), "exp_tab": (1.262, 2.0), "rsqrt_pos": (0.958, 1.5),
    "div_fast": (None, 1.0), "sqrt_pos": (None, 1.0),
}

_CTX = []


def ctx():
    if not _CTX:
        import gstpeaq_amd
        _CTX.append(gstpeaq_amd.Context(0))
    return _CTX[0]


def run(op, x, params=()):
    import gstpeaq_amd
    return gstpeaq_amd.debug_wave(ctx(), op, x, params)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------
def exact_pairs(fn, *args):
    """fn over the arguments in high precision -> (hi, lo): hi = the exact value rounded to double, lo = exact - hi
    rounded to double (the pair is good to ~2^-106 relative)"""
    n = len(args[0])
    hi, lo = np.empty(n), np.zeros(n)
    if mpmath is None:                                # pragma: no cover
        assert np.finfo(np.longdouble).nmant >= 63, "no mpmath and long double is not wider than double"
        v = fn(*[np.asarray(a, dtype=np.longdouble) for a in args], ld=True)
        hi[:] = v.astype(np.float64)
        with np.errstate(invalid="ignore"):
            lo[:] = np.where(np.isfinite(hi), (v - hi.astype(np.longdouble)).astype(np.float64), 0.)
        return hi, lo
    for i in range(n):
        e = fn(*[mpmath.mpf(float(a[i])) for a in args])
        h = float(e)
        hi[i] = h
        if math.isfinite(h):
            lo[i] = float(e - mpmath.mpf(h))
    return hi, lo


def _ld(name):
    return {"log": np.log, "exp": np.exp, "sqrt": np.sqrt}[name]


def f_log(x, ld=False):
    return _ld("log")(x) if ld else (mpmath.log(x) if x > 0 else (mpmath.mpf("-inf") if x == 0 else mpmath.nan))


def f_exp(x, ld=False):
    return _ld("exp")(x) if ld else mpmath.exp(x)


def f_sqrt(x, ld=False):
    return _ld("sqrt")(x) if ld else mpmath.sqrt(x)


def f_rsqrt(x, ld=False):
    return 1 / _ld("sqrt")(x) if ld else 1 / mpmath.sqrt(x)


def f_div(a, b, ld=False):
    return a / b


def f_pow(x, y, ld=False):
    return _ld("exp")(y * _ld("log")(x)) if ld else mpmath.exp(y * mpmath.log(x))


def ulp_errors(got, hi, lo):
    """|got - exact| / ulp(round(exact)) per element; infinite where one of the two is finite and the other not,
    or got is NaN"""
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(hi)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs((got - hi) - lo) / np.spacing(np.abs(np.where(fin, hi, 1.)))
    err = np.where(fin, err, np.where(got == hi, 0., np.inf))
    return np.where(np.isnan(got), np.inf, err)


_EXACT = {}


def exact_cached(key, fn, *args):
    if key not in _EXACT:
        _EXACT[key] = exact_pairs(fn, *args)
    return _EXACT[key]


def check(name, op, key, fn, args, bar=None, what=""):
    """runs op over args, prints the worst error and where, asserts it against the bar"""
    hi, lo = exact_cached(key, fn, *args)
    got = run(op, np.stack(args) if len(args) > 1 else args[0])
    err = ulp_errors(got, hi, lo)
    w = int(np.argmax(err))
    bar = BARS[name][1] if bar is None else bar
    print(f"\n[{op}] {what or key}: worst {err[w]:.3f} ulp at {[float(a[w]).hex() for a in args]} "
          f"(got {float(got[w])!r}, exact {float(hi[w])!r}; bar {np.max(bar):g}, {len(err)} arguments)")
    for b in np.unique(bar) if np.ndim(bar) and len(np.unique(bar)) <= 4 else ():   # ... and per class of bar
        k = np.flatnonzero(bar == b)
        j = k[int(np.argmax(err[k]))]
        print(f"    bar {b:g}: worst {err[j]:.3f} ulp at {[float(a[j]).hex() for a in args]} ({len(k)} arguments)")
    assert np.all(err <= bar), (op, key, float(err[w]), [float(a[w]).hex() for a in args])
    return got, err


# ---------------------------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------------------------
def positive_doubles(seed, n=N_SWEEP):
    """every finite positive magnitude, subnormals included: uniform over the bit patterns (log-uniform in value)"""
    rng = np.random.default_rng(seed)
    return rng.integers(1, 0x7FF0000000000000, size=n, dtype=np.uint64).view(np.float64)


def around_one(seed, n=N_SWEEP):
    """1 +- 2^-k u, k = 0 .. 51, u uniform in (0, 1)"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 52, size=n)
    u = 1. - rng.random(n)                            # (0, 1]
    s = np.where(rng.random(n) < .5, -1., 1.)
    x = 1. + s * np.ldexp(u, -k)
    return np.where(x > 0., x, 0.5)                   # (k = 0, u = 1, minus: 0 is not in log_pos's domain)


def log_uniform(seed, lo_exp, hi_exp, n=N_SWEEP, signed=False):
    rng = np.random.default_rng(seed)
    x = np.exp2(rng.uniform(lo_exp, hi_exp, size=n))
    return x * np.where(rng.random(n) < .5, -1., 1.) if signed else x


def step_ulps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def log_tab_edges():
    """for each of the 129 bins, in three binades -- [0.5, 1) and [1, 2), between which the fold at kLogTabFold switches
    the exponent that is counted, and a subnormal one --: the centre, both edges +- {0, 1, 2} ulp of the argument, and
    the all-ones fraction (whose index carries to 128)"""
    out = []
    for e in (0, 1, -1030):
        i = np.arange(129)
        pts = [np.ldexp((1. + i / 128.) / 2., e)]
        for edge in (np.ldexp((1. + (i - .5) / 128.) / 2., e), np.ldexp((1. + (i + .5) / 128.) / 2., e)):
            pts += [step_ulps(edge, k) for k in (-2, -1, 0, 1, 2)]
        pts.append(np.array([np.nextafter(np.ldexp(1., e), 0.)]))
        out.append(np.concatenate(pts))
    x = np.concatenate(out)
    assert np.all(x > 0)
    return x


def is_around_one(x):
    """bins 0 and 1 of log_tab's table in the binade of 1"""
    return (x >= 1.) & (x < 1. + 3. / 256.)


def exp_edges():
    """the rounding boundaries of rint in the argument reduction, n = -1280 .. 1280: (n + 1/2) ln 2 / 64 (exp_tab) and
    (n + 1/2) ln 2 (exp_fast), each +- {0, 1, 2} ulp; the smallest normal and the subnormal results; the clamp"""
    n = np.arange(-1280, 1281)
    pts = []
    for step in (math.log(2.) / 64., math.log(2.)):
        b = (n + .5) * step
        pts += [step_ulps(b, k) for k in (-2, -1, 0, 1, 2)]
    pts.append(np.random.default_rng(11).uniform(-745.2, -708., size=4096))
    pts.append(np.array([0., -0., -np.inf, 800., -800., 1000., -1000., 1000.0000001, -1000.0000001, 1e6, -1e6, 1e300,
                         -1e300, 709.782712893384, 709.782712893385, -745.1332191019411, -745.1332191019412]))
    return np.concatenate(pts)


# ---------------------------------------------------------------------------------------------------------------
# logarithms
# ---------------------------------------------------------------------------------------------------------------
LOG_OPS = ["log_pos", "log_nonneg", "log_tab", "log_tab_nonneg"]


def log_bar(op, x):
    if op.startswith("log_tab"):
        return np.where(is_around_one(x), BARS["log_tab@1"][1], BARS[op][1])
    return BARS[op][1]


@pytest.mark.parametrize("op", LOG_OPS)
def test_logarithm_against_the_exact_value(op):
    """Worst errors measured on the MI355X (ulp, against the exact value; peaq_wave.h's "<= 2 ulp", "<= 5 ulp
    around 1" were against OCML): log_pos = log_nonneg 1.894 at 0x1.00003fdd5d733p+0, log_tab = log_tab_nonneg 1.974 at
    0x1.fe9e25177b065p-1 outside [1, 1 + 3/256) and 5.035 at 0x1.00ffe78d8148dp+0 inside (BARS).
    Swept: every finite positive double (uniform over the bit patterns), 1 +- 2^-k u, the bin edges of the table form."""
    for key, x in (("log/all", positive_doubles(1)), ("log/one", around_one(2)), ("log/edges", log_tab_edges())):
        check(op, op, key, f_log, [x], bar=log_bar(op, x))


@pytest.mark.parametrize("op", LOG_OPS)
def test_logarithm_special_values(op):
    x = np.array([1., 2., .5, 4., np.nextafter(1., 2.), np.nextafter(1., 0.), TINY, np.finfo(float).max,
                  float.fromhex("0x1.00ffe78d8148dp+0"), float.fromhex("0x1.010001b476272p+0"),
                  float.fromhex("0x1.fe9e25177b065p-1"), float.fromhex("0x1.00ffa26f15e7dp+0")] * 16)
    got = run(op, x)
    assert got[0] == 0. and not np.signbit(got[0]), "ln 1 = 0 exactly"
    hi, lo = exact_pairs(f_log, x)
    assert np.all(ulp_errors(got, hi, lo) <= log_bar(op, x))
    if "nonneg" in op:
        y = run(op, np.array([0., np.inf, np.nan, 1.] * 16))
        assert np.all(y[0::4] == -np.inf) and np.all(y[1::4] == np.inf) and np.all(np.isnan(y[2::4])) and np.all(y[3::4] == 0.)
    if op.startswith("log_tab"):
        # NaN in -> NaN out, whatever its mantissa field says (the index is clamped into the table), and the kernel returns
        nans = np.array([0x7FF8000000000000, 0x7FFFFFFFFFFFFFFF, 0xFFF8000000000000, 0x7FF0000000000001,
                         0x7FF7FFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x7FFFE00000000000, 0x7FF8000000001FFF] * 8,
                        dtype=np.uint64).view(np.float64)
        assert np.all(np.isnan(run(op, nans)))


def test_log_scalar_constant_forms_are_bitwise_the_same():
    """peaq_wave.h: log_pos<true> = log_pos<false> with its constants in scalar registers, and log_nonneg_n<5> "the
    same operations in the same order as log_nonneg<true> ... bit for bit": five different arguments per lane, 0, +inf
    and subnormals among them"""
    x = np.concatenate([positive_doubles(1), around_one(2), log_tab_edges()])
    assert np.array_equal(bits(run("log_pos", x)), bits(run("log_pos_sk", x)))
    assert np.array_equal(bits(run("log_nonneg", x)), bits(run("log_nonneg_sk", x)))
    n = 1 << 14
    planes = np.stack([positive_doubles(21, n), around_one(22, n), positive_doubles(23, n), np.resize(log_tab_edges(), n),
                       positive_doubles(25, n)])
    rng = np.random.default_rng(26)
    for special in (0., np.inf, TINY, 5e-320, 1.):    # ... each at random places of every plane
        for p in range(5):
            planes[p, rng.integers(0, n, size=64)] = special
    got = run("log_nonneg_n5", planes)
    for p in range(5):
        assert np.array_equal(bits(got[p]), bits(run("log_nonneg_sk", planes[p]))), p
    assert np.any(got == -np.inf) and np.any(got == np.inf)


# ---------------------------------------------------------------------------------------------------------------
# exponentials
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["exp_fast", "exp_tab"])
def test_exponential_against_the_exact_value(op):
    """Worst errors measured on the MI355X: exp_fast 2.285 ulp at -0x1.2f407bf6050ffp+8, exp_tab 1.262 ulp at
    0x1.5bf5bafff56cdp+0 (BARS).  Swept: uniform on +-745 (overflow to +inf and the subnormal
    results included) and on +-40 (what the model feeds them), the rounding boundaries of both argument reductions,
    the clamp at +-1000."""
    rng = np.random.default_rng(3)
    for key, x in (("exp/745", rng.uniform(-745., 745., N_SWEEP)), ("exp/40", rng.uniform(-40., 40., N_SWEEP)),
                   ("exp/edges", exp_edges())):
        check(op, op, key, f_exp, [x])


@pytest.mark.parametrize("op", ["exp_fast", "exp_tab"])
def test_exponential_special_values(op):
    x = np.array([0., -0., -np.inf, 800., -800., 1000., -1000., 1e300, -1e300, -746., 709.8, -2000.] * 16)
    got = run(op, x).reshape(16, 12)
    assert np.all(got[:, 0] == 1.) and np.all(got[:, 1] == 1.), "e^0 = 1 exactly"
    assert np.all(got[:, [2, 4, 6, 8, 9, 11]] == 0.) and np.all(got[:, [3, 5, 7, 10]] == np.inf)


def test_exp_scalar_constant_forms_are_bitwise_the_same():
    """exp_fast<true> = exp_fast<false>, exp_fast_n<5> = exp_fast<true> element by element"""
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.uniform(-745., 745., N_SWEEP), rng.uniform(-40., 40., N_SWEEP), exp_edges()])
    assert np.array_equal(bits(run("exp_fast", x)), bits(run("exp_fast_sk", x)))
    n = 1 << 14
    planes = np.stack([rng.uniform(-745., 745., n), rng.uniform(-40., 40., n), rng.uniform(-1., 1., n),
                       np.resize(exp_edges(), n), rng.uniform(-745.2, -700., n)])
    for special in (0., -np.inf, 1000., -1000., 5e-320):
        for p in range(5):
            planes[p, rng.integers(0, n, size=64)] = special
    got = run("exp_fast_n5", planes)
    for p in range(5):
        assert np.array_equal(bits(got[p]), bits(run("exp_fast_sk", planes[p]))), p


# ---------------------------------------------------------------------------------------------------------------
# quotient, roots, powers
# ---------------------------------------------------------------------------------------------------------------
def test_div_fast_within_one_ulp():
    """peaq_wave.h: "<= 1 ulp" (a / b is correctly rounded where that was measured, so the claim stands as it is).
    a: +-2^+-100, b: +-2^+-200 as tools/check_math.hip; a = 0, a = b, b a power of two."""
    a, b = log_uniform(5, -100, 100, signed=True), log_uniform(6, -200, 200, signed=True)
    check("div_fast", "div_fast", "div/sweep", f_div, [a, b])
    n = 4096
    a2, b2 = log_uniform(7, -100, 100, n, signed=True), log_uniform(8, -200, 200, n, signed=True)
    got, _ = check("div_fast", "div_fast", "div/zero", f_div, [np.zeros(n), b2])
    assert np.all(got == 0.)
    check("div_fast", "div_fast", "div/equal", f_div, [b2, b2])
    p2 = np.ldexp(np.where(np.arange(n) % 2, -1., 1.), np.random.default_rng(9).integers(-200, 201, n))
    check("div_fast", "div_fast", "div/pow2", f_div, [a2, p2])


def test_sqrt_pos_within_one_ulp():
    """peaq_wave.h: "<= 1 ulp", "0 -> 0"; 2^+-600, 0, and the arguments below 2^-1000, subnormals included.  There
    the residual x - g^2 of the last correction falls below the subnormal spacing 2^-1074 and is rounded by up to
    2^-1075; times h = 1 / (2 sqrt x) that is 2^-1075 / (2 sqrt x), or 2^-1023 / x ulp of the result: the bound is
    1 + 2^-1023 / x ulp (measured on the MI355X with the claim of 1 ulp for all of them: 8.97 ulp at
    0x0.0c77d8840d9c4p-1022, bound 11.3; peaq_wave.h now states the bound)."""
    check("sqrt_pos", "sqrt_pos", "sqrt/sweep", f_sqrt, [log_uniform(10, -600, 600)])
    sub = np.concatenate([np.random.default_rng(12).integers(1, 1 << 52, size=4096, dtype=np.uint64).view(np.float64),
                          log_uniform(16, -1022, -990, 4096)])
    check("sqrt_pos", "sqrt_pos", "sqrt/tiny", f_sqrt, [sub], bar=1. + 2. ** -1023 / sub)
    z = run("sqrt_pos", np.zeros(256))
    assert np.all(z == 0.) and not np.any(np.signbit(z))
    check("sqrt_pos", "sqrt_pos", "sqrt/squares", f_sqrt, [np.arange(1., 4097.) ** 2])


def test_rsqrt_pos_against_the_exact_value():
    """peaq_wave.h: "<= 1 ulp or so"; worst measured on the MI355X: 0.958 ulp at 0x1.0f430b83d6951p-362 (BARS,
    DESIGN.md 4)"""
    check("rsqrt_pos", "rsqrt_pos", "rsqrt/sweep", f_rsqrt, [log_uniform(13, -600, 600)])
    check("rsqrt_pos", "rsqrt_pos", "rsqrt/pow4", f_rsqrt, [np.ldexp(1., 2 * np.arange(-300, 301))])


# op -> (bar of its logarithm per argument, bar of its exponential)
def pow_bar(op, x, y, lnx):
    if op == "pow_pos":
        e_log, e_exp = BARS["log_pos"][1], BARS["exp_fast"][1]
    else:
        e_log = np.where(is_around_one(x), BARS["log_tab@1"][1], BARS["log_tab"][1])
        e_exp = BARS["exp_tab" if op == "pow_tab" else "exp_fast"][1]
    return (e_log + .5) * np.abs(y * lnx) + e_exp


@pytest.mark.parametrize("op", ["pow_pos", "pow_tab", "pow_logtab"])
def test_pow_within_the_bound_derived_from_its_parts(op):
    """x^y = exp(y ln x): the logarithm's error and the rounding of the product, e_log + 1/2 ulp of y ln x, come out
    of the exponential as a relative error of the same size, on top of its own: (e_log + 1/2) |y ln x| + e_exp ulp.
    pow_pos is exp_fast(y log_pos(x)); pow_tab = exp_tab(y log_tab(x)) and pow_logtab = exp_fast(y log_tab(x)) are what
    the back ends call (peaq_backend.hip, GlobalTabs::pow and LdsTabs::pow) with y = 0.3 (modpatt.c:235) and 0.23
    (loudness) on excitations."""
    rng = np.random.default_rng(14)
    x, y = log_uniform(15, -60, 60), rng.uniform(0., 3., N_SWEEP)
    check(op, op, "pow/sweep", f_pow, [x, y], bar=pow_bar(op, x, y, np.log(x)))
    n = N_SWEEP // 4
    for k, yy in ((0, 0.3), (1, 0.23), (2, 0.1), (3, 0.4)):
        xe = np.exp(rng.uniform(math.log(1e-12), math.log(1e12), n))
        ye = np.full(n, yy)
        check(op, op, f"pow/{yy}", f_pow, [xe, ye], bar=pow_bar(op, xe, ye, np.log(xe)))


# ---------------------------------------------------------------------------------------------------------------
# cross-lane primitives
# ---------------------------------------------------------------------------------------------------------------
LANES = (0, 15, 16, 31, 32, 47, 48, 63, 37)


def families(seed, finite_only=True):
    """waves [W, 64] of the input families: (a) N(0,1); (b) magnitudes over 2^+-20 with random signs; (c) heavy
    cancellation; (d) a single non-zero lane at each of the 64 positions; (e) the lane index; (g) subnormals;
    and -0.0 at chosen lanes among N(0,1)"""
    rng = np.random.default_rng(seed)
    w = [rng.standard_normal((8, 64)),
         np.exp2(rng.uniform(-20, 20, (8, 64))) * np.where(rng.random((8, 64)) < .5, -1., 1.)]
    c = np.zeros((8, 64))
    for r in range(8):
        v = np.exp2(rng.uniform(0, 30, 24))
        row = np.concatenate([v, -v, rng.standard_normal(16) * 1e-6])
        c[r] = row[rng.permutation(64)]
    w.append(c)
    d = np.zeros((64, 64))
    d[np.arange(64), np.arange(64)] = rng.standard_normal(64) + 3.
    w.append(d)
    w.append(np.where(d != 0., -d, 0.))
    w.append(np.tile(np.arange(64.), (2, 1)))
    w.append(rng.integers(0, 1 << 52, (4, 64), dtype=np.uint64).view(np.float64) * np.where(rng.random((4, 64)) < .5, -1., 1.))
    z = rng.standard_normal((len(LANES), 64))
    z[np.arange(len(LANES)), LANES] = -0.
    w.append(z)
    return np.concatenate(w)


def frac_sum(v):
    return sum((Fraction(float(t)) for t in v), Fraction(0))


def assert_sums(got_lane_values, v, K, what):
    """|got - exact| <= K 2^-53 sum |v_j| in exact rational arithmetic; returns the K the data needed"""
    exact, mag = frac_sum(v), frac_sum(np.abs(v))
    worst = 0.
    for g in np.unique(got_lane_values):
        err = abs(Fraction(float(g)) - exact)
        assert err <= K * Fraction(U) * mag, (what, float(g), float(exact), float(err / (Fraction(U) * mag)) if mag else None)
        if mag:
            worst = max(worst, float(err / (Fraction(U) * mag)))
    return worst


def test_wave_sum():
    """K = 6: a term passes the six additions of the butterfly (lane bits 1, 2, 4, 8, 16, 32); every lane holds the
    bit-identical total"""
    w = families(30)
    got = run("wave_sum", w.reshape(-1)).reshape(w.shape)
    worst = 0.
    for r in range(len(w)):
        assert len(np.unique(bits(got[r]))) == 1, f"wave {r}: the lanes differ"
        worst = max(worst, assert_sums(got[r], w[r], 6, f"wave {r}"))
    print(f"\n[wave_sum] worst K = {worst:.3f} (bar 6)")
    for lane in LANES:                                # one +inf / one NaN: every lane says so
        v = np.random.default_rng(lane).standard_normal((2, 64))
        v[0, lane], v[1, lane] = np.inf, np.nan
        g = run("wave_sum", v.reshape(-1)).reshape(2, 64)
        assert np.all(g[0] == np.inf) and np.all(np.isnan(g[1])), lane


def test_wave_max():
    """exactly the maximum, in every lane; fmax semantics with NaN lanes (the maximum of the others)"""
    w = families(31)
    got = run("wave_max", w.reshape(-1)).reshape(w.shape)
    for r in range(len(w)):
        assert np.all(got[r] == np.max(w[r])), r
        if not (np.any(w[r] == 0.) and np.max(w[r]) == 0. and np.any(np.signbit(w[r][w[r] == 0.]))):
            assert len(np.unique(bits(got[r]))) == 1, r
    for lane in LANES:
        v = np.random.default_rng(100 + lane).standard_normal((3, 64))
        v[0, lane] = np.nan
        v[1, lane] = np.inf
        v[2, lane], v[2, (lane + 7) % 64] = np.nan, -np.inf
        g = run("wave_max", v.reshape(-1)).reshape(3, 64)
        assert np.all(g[0] == np.nanmax(v[0])) and np.all(g[1] == np.inf) and np.all(g[2] == np.nanmax(v[2])), lane


@pytest.mark.parametrize("op,planes", [("wave_sum2", 2), ("wave_sum4", 4)])
def test_wave_sum2_and_sum4(op, planes):
    """K = 6 additions on a term's path (one per shared half / row exchange, four inside the row); every lane holds
    the bit-identical totals; each total belongs to ITS plane: planes whose sums differ by orders of magnitude, a
    single non-zero lane in one plane at a time, and permuted planes give permuted totals"""
    w = families(32)
    W = len(w)
    rng = np.random.default_rng(33)
    scale = [1., 1e6, 1e-6, 1e12][:planes]
    x = np.stack([w[rng.permutation(W)] * scale[p] for p in range(planes)])          # [planes, W, 64]
    got = run(op, x.reshape(planes, -1)).reshape(planes, W, 64)
    worst = 0.
    for p in range(planes):
        for r in range(W):
            assert len(np.unique(bits(got[p, r]))) == 1, (p, r)
            worst = max(worst, assert_sums(got[p, r], x[p, r], 6, (op, p, r)))
    print(f"\n[{op}] worst K = {worst:.3f} (bar 6)")
    # a single non-zero lane, in one plane at a time: its value comes back in that plane, 0 in the others
    for p in range(planes):
        y = np.zeros((planes, 64, 64))
        y[p, np.arange(64), np.arange(64)] = np.arange(1., 65.) * (p + 1)
        g = run(op, y.reshape(planes, -1)).reshape(planes, 64, 64)
        for q in range(planes):
            assert np.array_equal(g[q], np.repeat(y[q].sum(axis=1), 64).reshape(64, 64)), (p, q)
    # permuted planes -> permuted totals, bit for bit (every slot adds its lanes up in the same tree, and additions
    # commute)
    perm = [1, 0] if planes == 2 else [2, 3, 1, 0]
    gp = run(op, x[perm].reshape(planes, -1)).reshape(planes, W, 64)
    for q, p in enumerate(perm):
        assert np.array_equal(bits(gp[q]), bits(got[p])), (op, "permuted", q, p)
    # non-finite lanes stay in their plane
    for lane in LANES:
        y = rng.standard_normal((planes, 2, 64))
        y[0, 0, lane], y[planes - 1, 1, lane] = np.inf, np.nan
        g = run(op, y.reshape(planes, -1)).reshape(planes, 2, 64)
        assert np.all(g[0, 0] == np.inf) and np.all(np.isnan(g[planes - 1, 1])), lane
        fin = np.ones((planes, 2), bool)
        fin[0, 0] = fin[planes - 1, 1] = False
        assert np.all(np.isfinite(g[fin])), lane


def test_wave_prefix_sum():
    """lane i = v_0 + ... + v_i.  K = 6: four additions inside the row of 16 (shifts by 1, 2, 4, 8) and the two row
    carries (lane 15 of the row before, lane 31)"""
    w = families(34)
    got = run("wave_prefix_sum", w.reshape(-1)).reshape(w.shape)
    worst = 0.
    for r in range(len(w)):
        exact, mag = Fraction(0), Fraction(0)
        for i in range(64):
            exact, mag = exact + Fraction(float(w[r, i])), mag + abs(Fraction(float(w[r, i])))
            err = abs(Fraction(float(got[r, i])) - exact)
            assert err <= 6 * Fraction(U) * mag, (r, i, float(got[r, i]), float(exact))
            worst = max(worst, float(err / (Fraction(U) * mag)) if mag else 0.)
    print(f"\n[wave_prefix_sum] worst K = {worst:.3f} (bar 6)")
    for lane in LANES:                                # a non-finite lane reaches the lanes >= it and no other
        for bad in (np.inf, np.nan):
            v = np.random.default_rng(lane).standard_normal(64)
            ref = run("wave_prefix_sum", v)
            v2 = v.copy()
            v2[lane] = bad
            g = run("wave_prefix_sum", v2)
            assert np.array_equal(bits(g[:lane]), bits(ref[:lane])) and not np.any(np.isfinite(g[lane:])), (lane, bad)


def lane_moves(op, x):
    if op == "lane_below":
        return np.concatenate([np.zeros((len(x), 1)), x[:, :-1]], axis=1)
    return np.concatenate([x[:, 1:], np.zeros((len(x), 1))], axis=1)


@pytest.mark.parametrize("op", ["lane_below", "lane_above"])
def test_lane_shifts_are_exact(op):
    """lane i <- lane i -+ 1, bit for bit (NaN payloads, -0.0, subnormals), +0.0 entering at lane 0 / 63"""
    x = np.random.default_rng(35).integers(0, 1 << 64, (16, 64), dtype=np.uint64, endpoint=False).view(np.float64)
    x[0, :8] = [-0., np.nan, np.inf, -np.inf, TINY, -TINY, 0., 1.]
    x[1, -8:] = [-0., np.nan, np.inf, -np.inf, TINY, -TINY, 0., 1.]
    got = run(op, x.reshape(-1)).reshape(x.shape)
    assert np.array_equal(bits(got), bits(lane_moves(op, x)))


def test_read_lane_broadcasts_bitwise():
    x = np.random.default_rng(36).integers(0, 1 << 64, (16, 64), dtype=np.uint64, endpoint=False).view(np.float64)
    for op, lane in (("read_lane_0", 0), ("read_lane_63", 63)):
        got = run(op, x.reshape(-1)).reshape(x.shape)
        assert np.array_equal(bits(got), np.repeat(bits(x[:, lane]), 64).reshape(x.shape)), op


def test_rows_transpose4_is_the_exact_permutation():
    """on return x[a] holds in row p what x[p] held in row a (lanes keep their place inside the row): 256 distinct
    64-bit patterns per wave, NaN payloads and -0.0 among them"""
    rng = np.random.default_rng(37)
    x = rng.integers(0, 1 << 64, (4, 8, 4, 16), dtype=np.uint64, endpoint=False)       # [register, wave, row, lane]
    x[0, 0, 0, :4] = np.array([0x8000000000000000, 0x7FF8000000000001, 0xFFF0000000000000, 0x7FF0000000000001], dtype=np.uint64)
    for wv in range(8):
        assert len(np.unique(x[:, wv])) == 256
    got = bits(run("rows_transpose4", x.view(np.float64).reshape(4, -1))).reshape(4, 8, 4, 16)
    assert np.array_equal(got, x.transpose(2, 1, 0, 3))


# ---- geometric scans ---------------------------------------------------------------------------------------------
K_SCAN = 32          # cap: <= 6 multiply-adds on a term's path plus the roundings of the powers that form its weight
                     # (an emulation that rounds more often than the kernel stays below 9.3); a lost row carry or a
                     # wrong power shows at K ~ 1e15


def ms_for(op):
    a109, a55 = (10. ** (-2.7 * 27. / 108.)) ** .4, (10. ** (-2.7 * 27. / 54.)) ** .4  # aLe of the two FFT band tables
    k_m1 = 1. - 0.993355506255034                                                        # slope filter (peaq_fb.hip)
    rng = np.random.default_rng(38)
    return [a109 * a109, a55 * a55, k_m1, 0.993355506255034, *rng.random(6), 1., 0., 1e-30, 1e-3, 1. - 2. ** -40]


def scan_reference(v, m, suffix):
    """exact recurrences R_i = m R_(i-1) + v_i and the same over |v| (160-bit arithmetic, good to 2^-150)"""
    mp = mpmath.mpf
    vv = [mp(float(t)) for t in (v[::-1] if suffix else v)]
    mm = mp(float(m))
    r, b, acc, accb = [], [], mp(0), mp(0)
    for t in vv:
        acc = mm * acc + t
        accb = mm * accb + abs(t)
        r.append(acc)
        b.append(accb)
    return (r[::-1], b[::-1]) if suffix else (r, b)


def assert_scan(op, got, v, m, suffix, u=U, tiny=TINY, lanes=range(64)):
    r, b = scan_reference(v, m, suffix)
    worst = 0.
    for i in lanes:
        err = abs(mpmath.mpf(float(got[i])) - r[i])
        # (+ 64 * the smallest subnormal: products that underflow lose up to half of it each, outside any relative bound)
        assert err <= K_SCAN * u * b[i] + 64 * tiny, (op, m, i, float(got[i]), float(r[i]), float(err / (u * b[i])) if b[i] else None)
        if b[i]:
            worst = max(worst, float((err - min(err, 64 * tiny)) / (u * b[i])))
    return worst


SCANS = [("wave_suffix_geometric", True), ("wave_prefix_geometric", False), ("wave_prefix_geometric_z", False),
         ("wave_prefix_geometric_f32", False)]


def run_scan(op, w, m):
    if op == "wave_prefix_geometric_z":
        return run(op, np.stack([w.reshape(-1)] * 3), [m])[0].reshape(w.shape)
    return run(op, w.reshape(-1), [m]).reshape(w.shape)


@pytest.mark.parametrize("op,suffix", SCANS)
def test_geometric_scans(op, suffix):
    """|got_i - sum_j m^|i-j| v_j| <= K u sum_j m^|i-j| |v_j| at every lane, K = 32 (see K_SCAN), u = 2^-53 (2^-24 for the
    FP32 overload, whose data and m are rounded to FP32 first); m: the constants of the kernels (aLe^2 of both band
    tables, the slope filter's 1 - A and A), random, 1 (plain sums), 0 (output = input), 1e-30 (m^16 underflows),
    1 - 2^-40"""
    f32 = op.endswith("f32")
    w = families(39)
    if f32:
        w = np.delete(w, slice(len(w) - 13, len(w) - 9), axis=0)     # (FP32 has no room for the FP64 subnormals of (g))
        w = w.astype(np.float32).astype(np.float64)
    worst = 0.
    some = np.r_[0:32, 32:len(w):5]                    # (the m's of no kernel: a share of the waves keeps the run short)
    for k, m in enumerate(ms_for(op)):
        w_all = w
        w = w_all if k < 4 or m in (1., 0., 1e-30) else w_all[some]
        got = run_scan(op, w, m)
        mr = float(np.float32(m)) if f32 else m
        for r in range(len(w)):
            worst = max(worst, assert_scan(op, got[r], w[r], mr, suffix, *((2. ** -24, 2. ** -149) if f32 else ())))
        if m == 0.:
            assert np.array_equal(got, w), "m = 0: output = input"
        w = w_all
    print(f"\n[{op}] worst K = {worst:.3f} (bar {K_SCAN})")


@pytest.mark.parametrize("op,suffix", SCANS)
def test_geometric_scans_keep_non_finite_lanes_where_the_recurrence_puts_them(op, suffix):
    """an inf or NaN at lane L reaches exactly the lanes >= L (prefix) / <= L (suffix); every other lane stays finite
    and within the bound -- no weight that happens to be 0 may be multiplied with a non-finite neighbour"""
    f32 = op.endswith("f32")
    rng = np.random.default_rng(40)
    for m in ms_for(op)[:5] + [1e-30]:
        mr = float(np.float32(m)) if f32 else m
        for lane in LANES:
            for bad in (np.inf, -np.inf, np.nan):
                v = rng.standard_normal(64)
                if f32:
                    v = v.astype(np.float32).astype(np.float64)
                v2 = v.copy()
                v2[lane] = bad
                got = run_scan(op, v2[None, :], m)[0]
                hit = range(0, lane + 1) if suffix else range(lane, 64)
                clean = [i for i in range(64) if i not in hit]
                assert not np.any(np.isfinite(got[list(hit)])), (op, m, lane, bad)
                assert np.all(np.isfinite(got[clean])), (op, m, lane, bad)
                v0 = v.copy()
                v0[lane] = 0.
                assert_scan(op, got, v0, mr, suffix, *((2. ** -24, 2. ** -149) if f32 else ()), lanes=clean)


def test_prefix_scan_with_kept_zero_registers_equals_the_plain_one():
    """dpp_rows_keep: "the other rows still read 0" -- three scans in a row through the SAME z15, z31 with different
    data (non-finite lanes in the first and the second among them) equal the plain overload bit for bit"""
    w = families(41)
    rng = np.random.default_rng(42)
    x = np.stack([w, w[rng.permutation(len(w))] * 1e3, w[rng.permutation(len(w))] * 1e-3])
    x[0, 3, 17], x[0, 4, 40], x[1, 5, 15], x[1, 6, 31], x[0, 7, 63], x[1, 8, 0] = np.inf, np.nan, np.nan, -np.inf, np.nan, np.inf
    for m in ms_for("z")[:6] + [1., 0., 1e-30]:
        got = run("wave_prefix_geometric_z", x.reshape(3, -1), [m])
        for p in range(3):
            assert np.array_equal(bits(got[p]), bits(run("wave_prefix_geometric", x[p].reshape(-1), [m]))), (m, p)


# ---- register DFTs -------------------------------------------------------------------------------------------------
def dft_inputs(n):
    """per lane n complex inputs: (a) N(0,1); (b) magnitudes over 2^+-20; unit impulses at every n (each reads off a row
    of twiddles), in the real and in the imaginary part; single complex exponentials at every k (read off the output
    order)"""
    rng = np.random.default_rng(43 + n)
    x = [rng.standard_normal((64, n)) + 1j * rng.standard_normal((64, n)),
         (np.exp2(rng.uniform(-20, 20, (64, n))) * np.exp(2j * np.pi * rng.random((64, n))))]
    imp = np.zeros((64, n), complex)
    for i in range(64):
        imp[i, i % n] = (1., 1j, -1., 1 + 1j)[(i // n) % 4]
    x.append(imp)
    k = np.arange(64) % n
    x.append(np.exp(2j * np.pi * np.outer(k, np.arange(n)) / n))
    return np.concatenate(x)                          # [lanes, n]


@pytest.mark.parametrize("n", [4, 8, 16])
def test_register_dfts(n):
    """X_k = sum_n x_n exp(-2 pi i n k / N) (the forward sign peaq_wave.h states), natural order in and out.
    Real and imaginary part each: |X_k - exact| <= K 2^-53 sum_n |x_n| with K = 8 by count: at most 4 levels of
    additions (dft16: two passes of dft4 with two levels each), 1 rounding each on partial sums that |x_n| bound, and
    one complex multiplication by a twiddle (c, s) good to 1/2 ulp: per part a product and a multiply-add (2
    roundings) plus the constant's 1/2, on |a.re| |c| + |a.im| |s| <= sqrt 2 |a| -- 4 + 2.5 sqrt 2 = 7.6, rounded
    up."""
    K = 8
    x = dft_inputs(n)
    planes = np.empty((2 * n, len(x)))
    planes[0::2], planes[1::2] = x.real.T, x.imag.T
    got = run(f"dft{n}", planes)
    X = got[0::2].T + 1j * got[1::2].T
    mp = mpmath
    tw = [mp.expjpi(mp.mpf(-2 * j) / n) for j in range(n)]
    worst = 0.
    for r in range(len(x)):
        xs = [mp.mpc(float(c.real), float(c.imag)) for c in x[r]]
        mag = sum(abs(c) for c in xs)
        for k in range(n):
            e = sum(xs[j] * tw[(j * k) % n] for j in range(n))
            err = max(abs(mp.mpf(float(X[r, k].real)) - e.real), abs(mp.mpf(float(X[r, k].imag)) - e.imag))
            assert err <= K * U * mag, (n, r, k, complex(X[r, k]), complex(e), float(err / (U * mag)))
            worst = max(worst, float(err / (U * mag)))
    print(f"\n[dft{n}] worst K = {worst:.3f} (bar {K})")
    # the exponentials of the last family land in bin k alone, bit-exact zeros aside: the output order
    tail = X[-64:]
    for i in range(64):
        assert np.argmax(np.abs(tail[i])) == i % n and abs(tail[i, i % n] - n) < 1e-13 * n, (n, i)
