"""The f64 elementary functions of csrc/device_rng.hpp, restated in plain Python -- the same constants, the same operations in
the same order, the tables read from csrc/rng_tables.inc -- and a reference layer in mpmath to hold them against.

Class A (u52, neg2_log_tab, sincos_2pi_tab, exp_tab and the loop:: spellings): chains of explicit fmas and exact bit
operations.  With a correctly rounded fma the restatement computes the device's bits; tests/test_elementary_functions.py
asserts that on the device.

Class B (div_fast, sqrt_fast, log_fast, log_factorial, tanh_abs_tab): the device starts from v_rcp_f64 / v_rsq_f64 seeds,
which no CPU reproduces, or holds sums the compiler may contract.  Here they use the correctly rounded `/` and sqrt; the
restatement bounds the scheme's own error, and the device is compared with mpmath directly.

exact(name, x) is the true value at 212 bits (an mpmath mpf), ulps(got, exact) the error of a binary64 result in units of
math.ulp(float(exact))."""
import math
import os
import re
import struct
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = os.path.join(ROOT, "simulatedannealingabc.jl_amd", "csrc", "rng_tables.inc")

HALF_BIN = 0x1000          # neg2_log_tab rounds the mantissa to 7 bits: the bin index is (t >> 13) & 127, half a bin is 1 << 12
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------- bits and the fused multiply-add
def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b & 0xFFFFFFFFFFFFFFFF))[0]


def hi_lo(x):
    b = bits(x)
    return b >> 32, b & M32


def from_hi_lo(hi, lo):
    return from_bits(((hi & M32) << 32) | (lo & M32))


def fma_fraction(a, b, c):
    """a b + c rounded once (Fraction.__float__ divides two integers, which is correctly rounded)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _fma_int(a, b, c):
    """The same value from integer arithmetic on the operands' mantissas: a fifth of the time of three Fractions."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)) or a == 0.0 or b == 0.0 or c == 0.0:
        return a * b + c                        # one rounding at the most: the product alone, or c alone
    ma, ea = math.frexp(a)
    mb, eb = math.frexp(b)
    mc, ec = math.frexp(c)
    p, ep = int(ma * 9007199254740992.0) * int(mb * 9007199254740992.0), ea + eb - 106
    q, eq = int(mc * 9007199254740992.0), ec - 53
    if ep >= eq:
        n, e = (p << (ep - eq)) + q, eq
    else:
        n, e = p + (q << (eq - ep)), ep
    if n == 0:
        return 0.0
    top = e + n.bit_length()                    # the result is in [2^(top - 1), 2^top)
    if n.bit_length() < 1000 and -1000 < top < 1000:
        return math.ldexp(float(n), e)          # int -> float rounds to nearest even; the scaling is exact for a normal result
    return fma_fraction(a, b, c)


fma = getattr(math, "fma", _fma_int)


# ---------------------------------------------------------------- the tables
def _read_tables():
    with open(TABLES, encoding="utf-8") as f:
        text = f.read()
    out = {}
    for name in ("kLogTab", "kSinCosTab", "kExp2Tab"):
        body = text.split(name, 1)[1].split("= {", 1)[1].split("\n};", 1)[0]
        body = "\n".join(line.split("//", 1)[0] for line in body.splitlines())
        out[name] = [float.fromhex(h) for h in re.findall(r"-?0x[0-9a-fA-F.]+p[+-]?\d+", body)]
    log_tab = [(out["kLogTab"][2 * i], out["kLogTab"][2 * i + 1]) for i in range(128)]
    sc = [(out["kSinCosTab"][2 * i], out["kSinCosTab"][2 * i + 1]) for i in range(32)]
    assert len(out["kLogTab"]) == 256 and len(out["kSinCosTab"]) == 64 and len(out["kExp2Tab"]) == 32
    return log_tab, sc + [sc[0]], out["kExp2Tab"]          # RngTables::sct has 33 rows, row 32 = row 0


LOG_TAB, SINCOS_TAB, EXP2_TAB = _read_tables()
LOG_FACTORIAL_TAB = [0.0, 0.0, 0.6931471805599453, 1.791759469228055, 3.1780538303479458, 4.787491742782046, 6.579251212010101,
                     8.525161361065415, 10.60460290274525, 12.801827480081469, 15.104412573075516, 17.502307845873887,
                     19.987214495661885, 22.552163853123425, 25.19122118273868, 27.89927138384089]

ONE_MINUS = float.fromhex("0x1.fffffffffffffp-1")
BIG = float.fromhex("0x1.8p52")
TWO_LN2 = 2.0 * 6.93147180559945309417e-01
PI_16 = 1.96349540849362077404e-01


# ---------------------------------------------------------------- class A
def u52(hi, lo):
    """(x + 1/2) 2^-52 of the 52 bits (low 20 of hi):(lo).  loop::u52 is the same expression with the exponent word in a register."""
    return from_hi_lo(0x3FF00000 | (hi & 0xFFFFF), lo) - ONE_MINUS


def _log_poly(s, nE, ey):
    p = 1.0 / 448.0
    p = fma(p, s, 1.0 / 192.0)
    p = fma(p, s, 1.0 / 80.0)
    p = fma(p, s, 1.0 / 32.0)
    p = fma(p, s, 1.0 / 12.0)
    p = fma(p, s, 0.25)
    l = fma(s * s, p, s)
    return fma(float(nE), TWO_LN2, ey) + l


def _log_bin(x, half_bin):
    hi, lo = hi_lo(x)
    t = (hi + half_bin) & M32
    tp = (t + (75 << 13)) & M32
    nE = 1023 - (tp >> 20)
    return hi, lo, nE, LOG_TAB[(t >> 13) & 127]


def neg2_log_tab_parts(x, half_bin=None):
    """(-2 log x, s): s is the polynomial's argument, whose range the header's remainder estimate rests on."""
    hi, lo, nE, (ex, ey) = _log_bin(x, HALF_BIN if half_bin is None else half_bin)
    m = from_hi_lo(hi + ((nE & M32) << 20), lo)                       # x 2^-E, exact
    s = fma(m, ex, 2.0)
    return _log_poly(s, nE, ey), s


def neg2_log_tab(x, half_bin=None):
    return neg2_log_tab_parts(x, half_bin)[0]


def loop_neg2_log_tab(x, half_bin=None):
    """loop::neg2_log_tab: the power of two goes into the table entry's exponent, not into x's."""
    hi, lo, nE, (ex, ey) = _log_bin(x, HALF_BIN if half_bin is None else half_bin)
    ehi, elo = hi_lo(ex)
    s = fma(x, from_hi_lo(ehi + ((nE & M32) << 20), elo), 2.0)
    return _log_poly(s, nE, ey)


def _sincos(u, tm):
    kf = tm - BIG
    r = PI_16 * fma(u, 32.0, -kf)
    sx, sy = SINCOS_TAB[hi_lo(tm)[1]]
    r2 = r * r
    p = 1.0 / 362880.0
    p = fma(p, r2, -1.0 / 5040.0)
    p = fma(p, r2, 1.0 / 120.0)
    p = fma(p, r2, -1.0 / 6.0)
    sr = fma(r * r2, p, r)
    q = 1.0 / 40320.0
    q = fma(q, r2, -1.0 / 720.0)
    q = fma(q, r2, 1.0 / 24.0)
    q = fma(q, r2, -0.5)
    q *= r2
    return sx + fma(sx, q, sy * sr), sy + fma(sy, q, -(sx * sr))


def sincos_2pi_tab(u):
    """(sin, cos) of 2 pi u, u in (0, 1)."""
    return _sincos(u, fma(u, 32.0, BIG))


def loop_sincos_2pi_tab(u):
    """loop::sincos_2pi_tab: 32 and 2^52 + 2^51 come from registers (loop::Regs), the operations are the same."""
    k32, big = 32.0, BIG
    return _sincos(u, fma(u, k32, big))


def exp_tab(x):
    x = min(max(x, -700.0), 700.0)
    tm = fma(x, float.fromhex("0x1.71547652b82fep+5"), BIG)
    nf = tm - BIG
    n = hi_lo(tm)[1]
    n = n - (1 << 32) if n & 0x80000000 else n                        # __double2loint: two's complement
    r = fma(-nf, float.fromhex("0x1.62e42feep-6"), x)
    r = fma(-nf, float.fromhex("0x1.a39ef35793c76p-38"), r)
    t = EXP2_TAB[n & 31]
    p = 1.0 / 720.0
    p = fma(p, r, 1.0 / 120.0)
    p = fma(p, r, 1.0 / 24.0)
    p = fma(p, r, 1.0 / 6.0)
    p = fma(p, r, 0.5)
    p = fma(p, r, 1.0)
    p = fma(p, r, 1.0)
    return math.ldexp(t * p, n >> 5)


# ---------------------------------------------------------------- class B (correctly rounded / and sqrt for the device's seeds)
def div_fast(a, b):
    return a / b


def sqrt_fast(x):
    return math.sqrt(x)


def log_fast(x):
    ix = bits(x)
    hx = ((ix >> 32) + 0x3ff00000 - 0x3fe6a09e) & M32
    hx = hx - (1 << 32) if hx & 0x80000000 else hx
    e = (hx >> 20) - 0x3ff
    hx = (hx & 0x000fffff) + 0x3fe6a09e
    m = from_hi_lo(hx, ix & M32)
    f = m - 1.0
    hfsq = 0.5 * f * f
    s = div_fast(f, 2.0 + f)
    z = s * s
    w = z * z
    t1 = w * fma(w, fma(w, 1.531383769920937332e-01, 2.222219843214978396e-01), 3.999999999940941908e-01)
    t2 = z * fma(w, fma(w, fma(w, 1.479819860511658591e-01, 1.818357216161805012e-01), 2.857142874366239149e-01),
                 6.666666666666735130e-01)
    R = t2 + t1
    dk = float(e)
    return fma(dk, 6.93147180369123816490e-01, (fma(s, hfsq + R, dk * 1.90821492927058770002e-10) - hfsq) + f)


def log_factorial(k):
    if k < 16.0:
        return LOG_FACTORIAL_TAB[int(k)]
    x = k + 1.0
    r = div_fast(1.0, x)
    r2 = r * r
    p = 1.0 / 1188.0
    p = fma(p, r2, -1.0 / 1680.0)
    p = fma(p, r2, 1.0 / 1260.0)
    p = fma(p, r2, -1.0 / 360.0)
    p = fma(p, r2, 1.0 / 12.0)
    return fma(x - 0.5, log_fast(x), -x) + fma(p, r, 9.18938533204672741780e-01)


def tanh_abs_tab(y):
    a = min(abs(y), 20.0)
    t = 1.0 - div_fast(2.0, exp_tab(2.0 * a) + 1.0)
    return math.copysign(t, y)


# ---------------------------------------------------------------- the reference
_MP = None


def mp():
    global _MP
    if _MP is None:
        import mpmath
        _MP = mpmath.mp.clone()
        _MP.prec = 212
    return _MP


def exact(name, x):
    """The true value of routine `name` at the binary64 argument(s) x, as an mpf of 212 bits.  x is a pair for div_fast (a, b)
    and u52 (hi, lo); sincos_2pi_tab gives the pair (sin, cos)."""
    c = mp()
    if name == "u52":
        return (c.mpf(((x[0] & 0xFFFFF) << 32) | x[1]) + c.mpf(0.5)) / c.mpf(2) ** 52
    if name == "div_fast":
        return c.mpf(x[0]) / c.mpf(x[1])
    v = c.mpf(x)
    if name in ("neg2_log_tab", "loop_neg2_log_tab"):
        return -2 * c.log(v)
    if name == "log_fast":
        return c.log(v)
    if name in ("sincos_2pi_tab", "loop_sincos_2pi_tab"):
        return c.sin(2 * c.pi * v), c.cos(2 * c.pi * v)
    if name == "exp_tab":
        return c.exp(min(max(v, c.mpf(-700)), c.mpf(700)))
    if name == "tanh_abs_tab":
        return c.tanh(v)
    if name == "log_factorial":
        return c.loggamma(v + 1)
    if name == "sqrt_fast":
        return c.sqrt(v)
    raise KeyError(name)


def ulps(got, ex):
    """|got - exact| in units of the spacing of binary64 at the exact value."""
    c = mp()
    return float(abs(c.mpf(got) - ex) / c.mpf(math.ulp(float(ex))))


def abs_units(got, ex):
    """|got - exact| in units of 2^-53: half an ulp of a result near 1 (sin, cos, tanh cross zero)."""
    c = mp()
    return float(abs(c.mpf(got) - ex) * c.mpf(2) ** 53)
