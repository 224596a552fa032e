"""The generator's f64 elementary functions (csrc/device_rng.hpp: u52, div_fast, sqrt_fast, log_fast, neg2_log_tab,
sincos_2pi_tab, exp_tab, tanh_abs_tab, log_factorial and the loop:: re-spellings) against exact arithmetic.

CPU: the restatement of tests/elementary_ref.py (same constants, operations and order, a correctly rounded fma) against mpmath
at 212 bits, on the inputs where such routines go wrong: bin boundaries and their binary64 neighbours, the table switch, the
neighbourhood of 1, multiples of the reduction step, the clamps.  GPU: one probe simulator applies each routine to its
argument; class A (chains of explicit fmas and exact bit operations) must give the restatement's bits, class B (hardware
reciprocal / reciprocal square root seeds, sums the compiler may contract) is held against mpmath directly.

Every bound, with what was measured.  Reference: mpmath, 212 bits.  Errors in ulps of the exact result; sincos_2pi_tab and
tanh_abs_tab absolutely, in units of 2^-53 (their results cross zero; the relative error near 0 is not controlled).  A CPU
bound is the restatement's worst error on the input sets of this module rounded up to the next 0.25 (the sets are samples: a
denser one finds slightly worse points); a device bound of class B is set by what the routine stands in for.

  routine         inputs                            bound  measured  where
  neg2_log_tab    uniform (0, 1)                     1.75     1.730  CPU restatement, ulp
  neg2_log_tab    bin boundaries (i + 1/2)/128       1.50     1.403  CPU restatement, ulp
  neg2_log_tab    bin boundaries (i + 1/4)/128       1.75     1.660  CPU restatement, ulp
  neg2_log_tab    near 1                             2.00     1.869  CPU restatement, ulp
  neg2_log_tab    1 + z^2, z ~ N(0, 2.5^2)           1.75     1.576  CPU restatement, ulp
  neg2_log_tab    uniform [1, 80]                    1.50     1.295  CPU restatement, ulp
  log_fast        uniform (0, 1)                     0.75     0.734  CPU restatement, ulp
  log_fast        bin boundaries (i + 1/2)/128       1.00     0.758  CPU restatement, ulp
  log_fast        bin boundaries (i + 1/4)/128       0.75     0.722  CPU restatement, ulp
  log_fast        near 1                             0.75     0.635  CPU restatement, ulp
  log_fast        1 + z^2, z ~ N(0, 2.5^2)           0.75     0.723  CPU restatement, ulp
  log_fast        uniform [1, 80]                    0.75     0.641  CPU restatement, ulp
  sincos_2pi_tab  uniform (0, 1)                     1.25     1.117  CPU restatement, x 2^-53
  sincos_2pi_tab  bin boundaries                     1.00     0.991  CPU restatement, x 2^-53
  sincos_2pi_tab  near 1                             0.50     0.500  CPU restatement, x 2^-53
  sincos_2pi_tab  k/32 + d                           1.00     0.906  CPU restatement, x 2^-53
  exp_tab         uniform [-700, 700]                2.00     1.755  CPU restatement, ulp
  exp_tab         uniform [-2, 2]                    2.00     1.792  CPU restatement, ulp
  exp_tab         edges                              1.25     1.073  CPU restatement, ulp
  log_factorial   k = 0..400                         1.75     1.572  CPU restatement, ulp
  log_factorial   large k                            1.75     1.548  CPU restatement, ulp
  tanh_abs_tab    uniform [-25, 25]                  2.25     2.081  CPU restatement, x 2^-53
  tanh_abs_tab    uniform [-1, 1]                    2.75     2.556  CPU restatement, x 2^-53
  tanh_abs_tab    edges                              0.75     0.745  CPU restatement, x 2^-53
  div_fast        2^-100 .. 2^100, both signs        0.50     0.500  CPU restatement, ulp
  div_fast        f / (2 + f) of log_fast            0.50     0.500  CPU restatement, ulp
  div_fast        2 / (e + 1) of tanh_abs_tab        0.50     0.500  CPU restatement, ulp
  div_fast        1 / x of log_factorial             0.50     0.500  CPU restatement, ulp
  sqrt_fast       log-uniform [1e-300, 1e300]        0.50     0.500  CPU restatement, ulp
  sqrt_fast       exact squares                      0.00     0.000  CPU restatement, ulp
  sqrt_fast       neighbours of exact squares        0.50     0.500  CPU restatement, ulp
  sqrt_fast       Box-Muller range (0, 75]           0.50     0.500  CPU restatement, ulp
  div_fast        all of its sets above              1.00     0.500  device (MI355X), ulp
  sqrt_fast       all of its sets above              1.00     0.500  device (MI355X), ulp
  log_fast        all of its sets above              1.00     0.726  device (MI355X), ulp
  log_factorial   all of its sets above              2.00     1.696  device (MI355X), ulp
  tanh_abs_tab    all of its sets above              3.06     2.556  device (MI355X), x 2^-53
  neg2_log_tab    max |s|, all of its sets           2^-7     1.000  CPU restatement, x 2^-7 (1.4995 with 0x800 added)

Class A on the device: bit for bit the restatement, both spellings, on all of the sets above."""
import functools
import math

import numpy as np
import pytest

from tests import elementary_ref as R

SEED = 20241220

# (routine, region) -> (bound, measured worst of the CPU restatement)
CPU_BOUNDS = {
    ("neg2_log_tab", "uniform (0, 1)"): (1.75, 1.730),
    ("neg2_log_tab", "bin boundaries (i + 1/2)/128"): (1.5, 1.403),
    ("neg2_log_tab", "bin boundaries (i + 1/4)/128"): (1.75, 1.660),
    ("neg2_log_tab", "near 1"): (2.0, 1.869),
    ("neg2_log_tab", "1 + z^2, z ~ N(0, 2.5^2)"): (1.75, 1.576),
    ("neg2_log_tab", "uniform [1, 80]"): (1.5, 1.295),
    ("log_fast", "uniform (0, 1)"): (0.75, 0.734),
    ("log_fast", "bin boundaries (i + 1/2)/128"): (1.0, 0.758),
    ("log_fast", "bin boundaries (i + 1/4)/128"): (0.75, 0.722),
    ("log_fast", "near 1"): (0.75, 0.635),
    ("log_fast", "1 + z^2, z ~ N(0, 2.5^2)"): (0.75, 0.723),
    ("log_fast", "uniform [1, 80]"): (0.75, 0.641),
    ("sincos_2pi_tab", "uniform (0, 1)"): (1.25, 1.117),
    ("sincos_2pi_tab", "bin boundaries"): (1.0, 0.991),
    ("sincos_2pi_tab", "near 1"): (0.5, 0.500),
    ("sincos_2pi_tab", "k/32 + d"): (1.0, 0.906),
    ("exp_tab", "uniform [-700, 700]"): (2.0, 1.755),
    ("exp_tab", "uniform [-2, 2]"): (2.0, 1.792),
    ("exp_tab", "edges"): (1.25, 1.073),
    ("log_factorial", "k = 0..400"): (1.75, 1.572),
    ("log_factorial", "large k"): (1.75, 1.548),
    ("tanh_abs_tab", "uniform [-25, 25]"): (2.25, 2.081),
    ("tanh_abs_tab", "uniform [-1, 1]"): (2.75, 2.556),
    ("tanh_abs_tab", "edges"): (0.75, 0.745),
    # the CPU's own '/' and sqrt: correctly rounded, half an ulp by definition (measured 0.500; exact squares 0)
    ("div_fast", "2^-100 .. 2^100, both signs"): (0.5, 0.500),
    ("div_fast", "f / (2 + f) of log_fast"): (0.5, 0.500),
    ("div_fast", "2 / (e + 1) of tanh_abs_tab"): (0.5, 0.500),
    ("div_fast", "1 / x of log_factorial"): (0.5, 0.500),
    ("sqrt_fast", "log-uniform [1e-300, 1e300]"): (0.5, 0.500),
    ("sqrt_fast", "exact squares"): (0.0, 0.000),
    ("sqrt_fast", "neighbours of exact squares"): (0.5, 0.500),
    ("sqrt_fast", "Box-Muller range (0, 75]"): (0.5, 0.500),
}
# routine -> (bound, measured worst on the device)
GPU_BOUNDS = {
    "div_fast": (1.0, 0.500),             # stands in for the compiler's correctly rounded '/'
    "sqrt_fast": (1.0, 0.500),            # ... and sqrt
    "log_fast": (1.0, 0.726),             # fdlibm documents its scheme below 1 ulp
    "log_factorial": (2.0, 1.696),        # the error of (x - 1/2) log x: an ulp or two of the result
    "tanh_abs_tab": (3.056, 2.556),       # the restatement's measured worst + 0.5 (the hardware divide's faithful rounding)
}
MAX_S = 2.0 ** -7                          # the premise of neg2_log_tab's remainder estimate


def neighbours(x):
    return [math.nextafter(x, -math.inf), x, math.nextafter(x, math.inf)]


def bin_boundaries(frac):
    return [v for E in (-3, -1, 0, 1, 4) for i in range(128) for v in neighbours(2.0 ** E * (1.0 + (i + frac) / 128.0))]


# ---------------------------------------------------------------- the input sets (region -> arguments)
@functools.lru_cache(maxsize=None)
def log_sets():
    rng = np.random.default_rng(SEED)
    z = rng.normal(0.0, 2.5, 3000)
    return {
        "uniform (0, 1)": rng.random(6000).tolist() + [2.0 ** -53, 1.0 - 2.0 ** -53, 0.5 - 2.0 ** -53, 0.5 + 2.0 ** -53],
        "bin boundaries (i + 1/2)/128": bin_boundaries(0.5),
        "bin boundaries (i + 1/4)/128": bin_boundaries(0.25),
        "near 1": [1.0 + s * 2.0 ** -k for k in range(6, 53) for s in (-1.0, 1.0)] + rng.uniform(0.99, 1.01, 3000).tolist()
                  + [v for E in (-1, 0) for v in neighbours(2.0 ** E * (1.0 + 52.5 / 128.0))],
        "1 + z^2, z ~ N(0, 2.5^2)": [R.fma(float(v), float(v), 1.0) for v in z],
        "uniform [1, 80]": rng.uniform(1.0, 80.0, 3000).tolist(),
    }


@functools.lru_cache(maxsize=None)
def sincos_sets():
    inside = lambda xs: [float(v) for v in xs if 0.0 < v < 1.0]
    ls = log_sets()
    d = [0.0, 2.0 ** -53, -2.0 ** -53] + [s * v for s in (1.0, -1.0) for v in neighbours(1.0 / 64.0)]
    return {
        "uniform (0, 1)": inside(ls["uniform (0, 1)"]),
        "bin boundaries": inside(ls["bin boundaries (i + 1/2)/128"] + ls["bin boundaries (i + 1/4)/128"]),
        "near 1": inside(ls["near 1"]),
        "k/32 + d": inside(k / 32.0 + dd for k in range(33) for dd in d),
    }


@functools.lru_cache(maxsize=None)
def exp_sets():
    rng = np.random.default_rng(SEED + 1)
    step = math.log(2.0) / 32.0
    return {
        "uniform [-700, 700]": rng.uniform(-700.0, 700.0, 8000).tolist(),
        "uniform [-2, 2]": rng.uniform(-2.0, 2.0, 8000).tolist(),
        "edges": [0.0, 1e-17, -1e-17, 700.0, -700.0, 712.5, -750.0]
                 + [n * step + d for n in (-33, -32, -1, 0, 1, 16, 31, 32) for d in (0.0, 1e-17, -1e-17, step / 2.0, -step / 2.0)],
    }


@functools.lru_cache(maxsize=None)
def log_factorial_sets():
    rng = np.random.default_rng(SEED + 2)
    return {
        "k = 0..400": [float(k) for k in range(401)],
        "large k": [15.0, 16.0, 17.0, 1e3, 1e4, 1e6, 2.0 ** 30] + [float(k) for k in rng.integers(16, 2 ** 30, 2000, endpoint=True)],
    }


@functools.lru_cache(maxsize=None)
def tanh_sets():
    rng = np.random.default_rng(SEED + 3)
    return {
        "uniform [-25, 25]": rng.uniform(-25.0, 25.0, 9000).tolist(),
        "uniform [-1, 1]": rng.uniform(-1.0, 1.0, 9000).tolist(),
        "edges": [1e-9, -1e-9, 19.99, 20.0, 25.0, -19.99, -20.0, -25.0],
    }


@functools.lru_cache(maxsize=None)
def div_sets():
    rng = np.random.default_rng(SEED + 4)
    mag = lambda n: rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-100, 100, n, endpoint=True)
    f = rng.uniform(-0.293, 0.414, 4000)
    e = [R.exp_tab(2.0 * float(a)) for a in rng.uniform(0.0, 20.0, 3000)]
    x = [float(k) + 1.0 for k in range(16, 417)] + [float(k) + 1.0 for k in rng.integers(16, 2 ** 30, 2600, endpoint=True)]
    return {
        "2^-100 .. 2^100, both signs": list(zip(map(float, mag(6000)), map(float, mag(6000)))),
        "f / (2 + f) of log_fast": [(float(v), 2.0 + float(v)) for v in f],
        "2 / (e + 1) of tanh_abs_tab": [(2.0, v + 1.0) for v in e],
        "1 / x of log_factorial": [(1.0, v) for v in x],
    }


@functools.lru_cache(maxsize=None)
def sqrt_sets():
    rng = np.random.default_rng(SEED + 5)
    roots = [float(n) * 2.0 ** int(j) for n, j in zip(rng.integers(1, 2 ** 26, 2000), rng.integers(-40, 40, 2000))]
    squares = [r * r for r in roots]                                   # exact: the roots have 26 bits
    return {
        "log-uniform [1e-300, 1e300]": [float(v) for v in 10.0 ** rng.uniform(-300.0, 300.0, 6000)],
        "exact squares": squares,
        "neighbours of exact squares": [v for s in squares for v in (math.nextafter(s, 0.0), math.nextafter(s, math.inf))],
        "Box-Muller range (0, 75]": [75.0] + [float(v) for v in rng.uniform(0.0, 75.0, 5000) if v > 0.0],
    }


@functools.lru_cache(maxsize=None)
def u52_words():
    """(hi, lo) pairs: the corners of the 52 bits under several settings of the 12 bits u52 must mask off, and random words."""
    rng = np.random.default_rng(SEED + 6)
    corners = [(h | top, lo) for h in (0, 1, 0xFFFFF, 0x80000) for lo in (0, 1, 0xFFFFFFFF) for top in (0, 0xFFF00000, 0x40000000)]
    return corners + [(int(h), int(lo)) for h, lo in rng.integers(0, 2 ** 32, (3000, 2))]


def flat(sets):
    return [v for xs in sets.values() for v in xs]


# ---------------------------------------------------------------- restatement and reference, each computed once
@functools.lru_cache(maxsize=None)
def restated(name):
    """{argument: the restatement's result} over the routine's input sets."""
    if name in ("neg2_log_tab", "loop_neg2_log_tab"):
        return {x: getattr(R, name)(x) for x in flat(log_sets())}
    if name == "log_fast":
        return {x: R.log_fast(x) for x in flat(log_sets())}
    if name in ("sincos_2pi_tab", "loop_sincos_2pi_tab"):
        return {u: getattr(R, name)(u) for u in flat(sincos_sets())}
    sets = {"exp_tab": exp_sets, "log_factorial": log_factorial_sets, "tanh_abs_tab": tanh_sets, "sqrt_fast": sqrt_sets}
    if name == "div_fast":
        return {ab: R.div_fast(*ab) for ab in flat(div_sets())}
    return {x: getattr(R, name)(x) for x in flat(sets[name]())}


@functools.lru_cache(maxsize=None)
def exact_values(name):
    """{argument: the true value} over the routine's input sets (the two logs share theirs)."""
    if name == "neg2_log_tab":
        return {x: -2 * v for x, v in exact_values("log_fast").items()}
    sets = {"log_fast": log_sets, "sincos_2pi_tab": sincos_sets, "exp_tab": exp_sets, "log_factorial": log_factorial_sets,
            "tanh_abs_tab": tanh_sets, "sqrt_fast": sqrt_sets, "div_fast": div_sets}
    return {x: R.exact(name, x) for x in set(flat(sets[name]()))}


def worst(name, region, xs, got, measure=R.ulps, part=None):
    """The largest error of got[x] over xs against the exact values, printed with its argument."""
    ex = exact_values(name)
    err, arg = max((measure(got[x] if part is None else got[x][part], ex[x] if part is None else ex[x][part]), x) for x in xs)
    unit = "ulp" if measure is R.ulps else "x 2^-53"
    what = name if part is None else f"{name}[{('sin', 'cos')[part]}]"
    print(f"{what:26s} {region:34s} {len(xs):6d} points: worst {err:.3f} {unit} at {arg!r}")
    return err


def check_cpu(name, sets, measure=R.ulps, restatement=None, parts=(None,)):
    got = restated(restatement or name)
    bad = []
    for region, xs in sets.items():
        err = max(worst(name, region, xs, got, measure, part) for part in parts)
        bound, _ = CPU_BOUNDS[(name, region)]
        if not err <= bound:
            bad.append(f"{name}, {region}: {err:.3f} > {bound}")
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------- CPU
def test_the_integer_fma_is_correctly_rounded():
    """elementary_ref's fma (Python 3.10 has no math.fma) against float(Fraction(a) Fraction(b) + Fraction(c)), cancellation
    to the last bit and far-apart exponents included."""
    rng = np.random.default_rng(SEED + 7)
    for i in range(4000):
        a, b = (float(rng.uniform(-2, 2)) * 2.0 ** int(rng.integers(-300, 300)) for _ in range(2))
        c = -a * b * (1.0 + float(rng.choice([0.0, 2.0 ** -52, 1e-8, 1.0]))) if i % 2 else \
            float(rng.uniform(-2, 2)) * 2.0 ** int(rng.integers(-600, 600))
        assert R._fma_int(a, b, c) == R.fma_fraction(a, b, c), (a, b, c)
    assert R._fma_int(3.0, 0.0, -0.0) == 0.0 and R._fma_int(2.0 ** -600, 2.0 ** -600, 1.0) == 1.0


def test_u52_is_exact():
    for hi, lo in u52_words():
        got = R.u52(hi, lo)
        assert R.mp().mpf(got) == R.exact("u52", (hi, lo)) and 0.0 < got < 1.0, (hi, lo)


def test_neg2_log_tab_restatement_within_bounds():
    check_cpu("neg2_log_tab", log_sets())


def test_the_two_spellings_give_equal_bits():
    a, b = restated("neg2_log_tab"), restated("loop_neg2_log_tab")
    assert len(a) > 15000 and all(R.bits(a[x]) == R.bits(b[x]) for x in a)
    a, b = restated("sincos_2pi_tab"), restated("loop_sincos_2pi_tab")
    assert len(a) > 8000 and all(R.bits(a[u][0]) == R.bits(b[u][0]) and R.bits(a[u][1]) == R.bits(b[u][1]) for u in a)


def test_neg2_log_tab_polynomial_argument_stays_within_the_remainder_estimate():
    """|s| <= 2^-7 is what the header derives the polynomial's remainder from: rounding the mantissa to its 7 leading bits
    must put x within HALF a bin of the bin's centre (with a quarter of a bin added instead, |s| reaches 1.5 x 2^-7)."""
    s, x = max((abs(R.neg2_log_tab_parts(x)[1]), x) for x in flat(log_sets()))
    print(f"neg2_log_tab: max |s| = {s * 128.0:.4f} x 2^-7 at {x!r}")
    assert s <= MAX_S
    assert R.neg2_log_tab_parts(1.0)[1] == 0.0 and R.neg2_log_tab(1.0) == 0.0        # 1 is a bin centre


def test_log_fast_restatement_within_bounds():
    check_cpu("log_fast", log_sets())


def test_sincos_2pi_tab_restatement_within_bounds():
    check_cpu("sincos_2pi_tab", sincos_sets(), measure=R.abs_units, parts=(0, 1))


def test_sincos_2pi_tab_returns_the_table_at_multiples_of_a_32nd():
    for k in range(1, 32):
        assert R.sincos_2pi_tab(k / 32.0) == R.SINCOS_TAB[k] == R.loop_sincos_2pi_tab(k / 32.0)
    assert [R.sincos_2pi_tab(k / 32.0) for k in (8, 16, 24)] == [(1.0, 0.0), (0.0, -1.0), (-1.0, 0.0)]


def test_exp_tab_restatement_within_bounds():
    check_cpu("exp_tab", exp_sets())
    assert R.exp_tab(712.5) == R.exp_tab(700.0) and R.exp_tab(-750.0) == R.exp_tab(-700.0) and R.exp_tab(0.0) == 1.0


def test_log_factorial_restatement_within_bounds():
    check_cpu("log_factorial", log_factorial_sets())
    for k in range(16):
        assert R.ulps(R.LOG_FACTORIAL_TAB[k], R.mp().loggamma(k + 1)) <= 0.5, k          # the table is correctly rounded


def test_tanh_abs_tab_restatement_within_bounds():
    check_cpu("tanh_abs_tab", tanh_sets(), measure=R.abs_units)
    assert R.tanh_abs_tab(-25.0) == -R.tanh_abs_tab(20.0) == -1.0


def test_div_and_sqrt_references_are_correctly_rounded():
    """The restatement of class B stands on the CPU's '/' and sqrt: half an ulp, which also checks exact() and ulps()."""
    check_cpu("div_fast", div_sets())
    check_cpu("sqrt_fast", sqrt_sets())
    got = restated("sqrt_fast")
    assert all(got[s] * got[s] == s for s in sqrt_sets()["exact squares"])


# ---------------------------------------------------------------- GPU
# theta = (x > 0, y in [-700, 700], u in (0, 1), b != 0); rho[j] = one routine of its argument.  x < 0 (the quotients' second
# sign) must not index log_factorial's table.  14 values in 17 statistics: above 16 a source is compiled into the wide form of
# the launch chain's kernels, which has no one-launch variants -- the compile-only check below takes an eighth of the time.
PROBE_SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const double x = theta[0], y = theta[1], u = theta[2], b = theta[3];
  const sabc::loop::Regs c = sabc::loop::Regs::load();
  const uint32_t hi = (uint32_t)__double2hiint(b), lo = (uint32_t)__double2loint(b);
  rho[0] = sabc::u52(hi, lo);
  rho[1] = sabc::loop::u52(hi, lo, c);
  rho[2] = sabc::neg2_log_tab(x);
  rho[3] = sabc::loop::neg2_log_tab(x);
  sabc::sincos_2pi_tab(u, rho[4], rho[5]);
  sabc::loop::sincos_2pi_tab(u, rho[6], rho[7], c);
  rho[8] = sabc::exp_tab(y);
  rho[9] = sabc::div_fast(x, b);
  rho[10] = sabc::sqrt_fast(x);
  rho[11] = sabc::log_fast(x);
  rho[12] = x >= 0.0 ? sabc::log_factorial(x) : 0.0;
  rho[13] = sabc::tanh_abs_tab(y);
  rho[14] = rho[15] = rho[16] = 0.0;
}
"""
PROBE_STATS = 17
MAX_LAUNCH = 20000


def word_carrier(hi, lo):
    """A finite, normal double whose two words are (hi, lo) but for the exponent field, which u52 masks off anyway."""
    e = (hi >> 20) & 0x7FF
    return R.from_hi_lo(hi if 0 < e < 0x7FF else (hi & 0x800FFFFF) | (0x400 << 20), lo)


def test_the_probe_source_compiles_without_a_device(S):
    assert S.DeviceSource(PROBE_SRC, 4, PROBE_STATS).compile_check()


@pytest.fixture(scope="module")
def probe(S, gpu):
    """Three launches of the probe over the input sets, a set shorter than its launch padded with its last element:
    {routine: {argument: the device's result}}."""
    with pytest.MonkeyPatch.context() as env:
        env.setenv("SABC_PERSISTENT", "0")              # the launch chain's kernels only
        h = S.SabcHandle(n_particles=256, model=S.DeviceSource(PROBE_SRC, 4, PROBE_STATS),
                         prior=S.product_distribution([S.Uniform(0.0, 1.0)] * 4), seed=SEED)

    def launch(x=(1.0,), y=(0.0,), u=(0.5,), b=(1.0,)):
        m = max(len(x), len(y), len(u), len(b))
        assert m <= MAX_LAUNCH
        theta = np.array([list(col) + [col[-1]] * (m - len(col)) for col in (x, y, u, b)], dtype=np.float64)
        assert np.isfinite(theta).all() and (theta[2] > 0.0).all() and (theta[2] < 1.0).all() and (theta[3] != 0.0).all()
        assert (np.abs(theta[1]) <= 750.0).all()
        rho = h.simulate(theta, 0, 0)
        assert rho.shape == (PROBE_STATS, m)
        return rho

    out = {}
    xs, ys, us, ws = flat(log_sets()), flat(exp_sets()), flat(sincos_sets()), u52_words()
    rho = launch(xs, ys, us, [word_carrier(*w) for w in ws])
    out["u52"] = dict(zip(ws, rho[0]))
    out["loop_u52"] = dict(zip(ws, rho[1]))
    out["neg2_log_tab"] = dict(zip(xs, rho[2]))
    out["loop_neg2_log_tab"] = dict(zip(xs, rho[3]))
    out["sincos_2pi_tab"] = dict(zip(us, zip(rho[4], rho[5])))
    out["loop_sincos_2pi_tab"] = dict(zip(us, zip(rho[6], rho[7])))
    out["exp_tab"] = dict(zip(ys, rho[8]))
    out["log_fast"] = dict(zip(xs, rho[11]))
    xs, ys = flat(sqrt_sets()), flat(tanh_sets())
    rho = launch(xs, ys)
    out["sqrt_fast"] = dict(zip(xs, rho[10]))
    out["tanh_abs_tab"] = dict(zip(ys, rho[13]))
    ab, ks = flat(div_sets()), flat(log_factorial_sets())
    rho = launch([a for a, _ in ab] + ks, b=[b for _, b in ab])
    out["div_fast"] = dict(zip(ab, rho[9]))
    out["log_factorial"] = dict(zip(ks, rho[12, len(ab):]))
    h.close()
    return out


def as_bits(values):
    return np.array([R.bits(float(v)) for v in values], dtype=np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["neg2_log_tab", "loop_neg2_log_tab", "sincos_2pi_tab", "loop_sincos_2pi_tab", "exp_tab"])
def test_device_class_a_equals_the_restatement_bit_for_bit(probe, name):
    want, got = restated(name), probe[name]
    args = list(want)
    assert len(args) > 50 and set(args) == set(got)
    if name.endswith("sincos_2pi_tab"):
        for part in (0, 1):
            np.testing.assert_array_equal(as_bits(got[u][part] for u in args), as_bits(want[u][part] for u in args))
    else:
        np.testing.assert_array_equal(as_bits(got[x] for x in args), as_bits(want[x] for x in args))


@pytest.mark.gpu
def test_device_u52_equals_the_restatement_bit_for_bit(probe):
    words = u52_words()
    want = as_bits(R.u52(hi, lo) for hi, lo in words)
    np.testing.assert_array_equal(as_bits(probe["u52"][w] for w in words), want)
    np.testing.assert_array_equal(as_bits(probe["loop_u52"][w] for w in words), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["div_fast", "sqrt_fast", "log_fast", "log_factorial", "tanh_abs_tab"])
def test_device_class_b_within_bounds_of_exact(probe, name):
    sets = {"div_fast": div_sets, "sqrt_fast": sqrt_sets, "log_fast": log_sets, "log_factorial": log_factorial_sets,
            "tanh_abs_tab": tanh_sets}[name]()
    measure = R.abs_units if name == "tanh_abs_tab" else R.ulps
    bound = GPU_BOUNDS[name][0]
    if name == "tanh_abs_tab":
        assert bound == pytest.approx(max(CPU_BOUNDS[(name, region)][1] for region in sets) + 0.5)
    err = max(worst(name, "device, " + region, xs, probe[name], measure) for region, xs in sets.items())
    if name in ("div_fast", "sqrt_fast"):
        ex, args = exact_values(name), flat(sets)
        off = sum(measure(probe[name][x], ex[x]) > 0.5 for x in args)
        print(f"{name}: {off} of {len(args)} results ({100.0 * off / len(args):.2f} %) are not the correctly rounded one")
    assert err <= bound, f"{name}: {err:.3f} > {bound}"
