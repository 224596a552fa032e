"""The binary32 draws of csrc/device_rng.hpp (namespace f32: box_muller_quad, uniform_quad) restated in NumPy float32 -- the
same constants, the same operations in the same order, the tables read from csrc/rng_tables.inc and rounded to binary32 as the
device's conversion rounds them.  Every step is class A in the terms of tests/elementary_ref.py: an exact bit operation, a
table read, an fma / mul / add of binary32 or the correctly rounded square root, so with a correctly rounded fma this file
computes the device's bits (tests/test_gpu_f32_draws.py asserts that on the device).

The fma.  NumPy has none, and float32(float64(a) * float64(b) + float64(c)) rounds twice: the product is exact in binary64,
the sum is not, and where the rounded sum lands on the midpoint of two binary32 numbers the second rounding goes the wrong
way.  fma32 rounds the sum TO ODD in binary64 (the two-sum error term says on which side of the rounded sum the exact one
lies), after which the rounding to binary32 is the correct one: 53 bits are more than 24 + 2.  fma32_exact is the scalar
check of it in exact rationals (tests/test_f32_draws.py).

Vectorised: words are uint32 arrays of shape (n, 4), the results float32 arrays of shape (n, 4)."""
import math
import struct
from fractions import Fraction

import numpy as np

from tests import elementary_ref as R

F = np.float32
LOG_X = np.array([e[0] for e in R.LOG_TAB]).astype(F)          # -2 inv_i, rounded to binary32 (v_cvt_f32_f64: nearest even)
LOG_Y = np.array([e[1] for e in R.LOG_TAB]).astype(F)          # -2 log c_i
SIN = np.array([e[0] for e in R.SINCOS_TAB]).astype(F)         # 33 rows
COS = np.array([e[1] for e in R.SINCOS_TAB]).astype(F)

TWO_LN2 = F(float.fromhex("0x1.62e43p+0"))
PI_16_SCALED = F(float.fromhex("0x1.921fb6p-30"))              # (pi / 16) 2^-27
PI_16_HALF = F(float.fromhex("-0x1.921fb6p-4"))                # -(pi / 16) / 2
Z_MAX = float(np.sqrt(66.0 * np.log(2.0)))                     # u = 2^-33


def fma32(a, b, c):
    """a b + c of binary32 arrays, rounded once."""
    a, b, c = (np.asarray(v, dtype=F).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(all="ignore"):                            # a simulated path may blow up: inf and NaN pass through
        return _fma32(a, b, c)


def _fma32(a, b, c):
    p = a * b                                                  # exact: 48 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                            # exact sum = s + err
    inexact = err != 0.0
    # towards zero where the rounding went away from it ...
    away = inexact & ((err < 0.0) == (s > 0.0)) & (s != 0.0)
    bits = s.view(np.int64).copy()
    bits = np.where(away, bits - 1, bits)                      # the magnitude's next number below (sign-magnitude layout)
    # ... and the last bit set where the sum was not exact: round to odd
    bits = np.where(inexact, bits | 1, bits)
    return bits.view(np.float64).astype(F)


def round_fraction_to_f32(q):
    """The binary32 number nearest to the rational q, ties to even (normal range)."""
    if q == 0:
        return F(0.0)
    near = F(float(q))
    cands = sorted({near, np.nextafter(near, F(np.inf)), np.nextafter(near, F(-np.inf))}, key=float)
    best = min(cands, key=lambda v: (abs(Fraction(float(v)) - q), int(np.array(v).view(np.uint32)) & 1))
    return best


def fma32_exact(a, b, c):
    return round_fraction_to_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _u32(x):
    return np.asarray(x).astype(np.uint32)


def radius_uniform(a):
    """u = fma((float)a, 2^-32, 2^-33) of uint32 words: in [2^-33, 1]."""
    return fma32(_u32(a).astype(F), F(2.0 ** -32), F(2.0 ** -33))


def neg2_log(u):
    """f32::neg2_log: -2 log(u), u in [2^-33, 1]."""
    u = np.asarray(u, dtype=F)
    bits = u.view(np.uint32)
    t = bits + np.uint32(0x8000)
    tp = t + np.uint32(75 << 16)
    nE = np.uint32(127) - (tp >> np.uint32(23))
    i = (t >> np.uint32(16)) & np.uint32(127)
    c = (t & np.uint32(0xFFFF0000)).view(F)
    ex = (LOG_X[i].view(np.uint32) + (nE << np.uint32(23))).view(F)
    ey = LOG_Y[i]
    s = (u - c) * ex
    p = fma32(s, F(1.0) / F(32.0), F(1.0) / F(12.0))
    p = fma32(p, s, F(0.25))
    l = fma32(s * s, p, s)
    return fma32(nE.astype(np.int32).astype(F), TWO_LN2, ey) + l


def sincos_turns(b):
    """(sin, cos) of 2 pi (b >> 8) 2^-24 as f32::box_muller_quad computes them from the angle word b."""
    t2 = _u32(b) + np.uint32(0x04000000)
    fi = t2 & np.uint32(0x07FFFF00)
    k = t2 >> np.uint32(27)
    S, C = SIN[k], COS[k]
    r = fma32(fi.astype(F), PI_16_SCALED, PI_16_HALF)
    r2 = r * r
    sr = fma32(r * r2, fma32(r2, F(1.0) / F(120.0), F(-1.0) / F(6.0)), r)
    q = fma32(r2, F(1.0) / F(24.0), F(-0.5)) * r2
    sn = fma32(C, sr, fma32(S, q, S))
    cs = fma32(-S, sr, fma32(C, q, C))
    return sn, cs


def pair(a, b):
    """(z0, z1) of the words (a, b): the radius from a, the angle from b."""
    rad = np.sqrt(neg2_log(radius_uniform(a)))                 # IEEE: correctly rounded
    sn, cs = sincos_turns(b)
    return fma32(rad, cs, F(0.0)), fma32(rad, sn, F(0.0))


def box_muller_quad(w):
    """The four normals of each block of w[n, 4] (uint32)."""
    w = _u32(w).reshape(-1, 4)
    z0, z1 = pair(w[:, 0], w[:, 1])
    z2, z3 = pair(w[:, 2], w[:, 3])
    return np.stack([z0, z1, z2, z3], axis=1)


def uniform_quad(w):
    """The four uniforms of each block: ((w_i >> 9) + 1/2) 2^-23, exact."""
    w = _u32(w).reshape(-1, 4)
    return fma32((w >> np.uint32(9)).astype(F), F(2.0 ** -23), F(2.0 ** -24))


def blocks(O, seed, pid, purpose, it, k0, n):
    """Blocks k0 .. k0 + n - 1 of a stream as uint32[n, 4], from the oracle's Philox."""
    return np.array([O.stream_block(seed, pid, purpose, it, k0 + j) for j in range(n)], dtype=np.uint32).reshape(n, 4)


def philox_blocks(seed, pid, purpose, it, k):
    """stream_block (csrc/device_rng.hpp) in NumPy, vectorised over pid and k (broadcast against each other): uint32[..., 4].
    Held against the oracle's Philox by tests/test_f32_draws.py."""
    pid, k = np.broadcast_arrays(np.asarray(pid, dtype=np.uint64), np.asarray(k, dtype=np.uint64))
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1 = pid & m32, k & m32
    c2 = np.full(pid.shape, int(it) & 0xFFFFFFFF, dtype=np.uint64)
    c3 = np.uint64(purpose & 0xFF) | (((pid >> np.uint64(32)) << np.uint64(8)) & m32) | np.uint64(((int(it) >> 32) & 0xFF) << 24)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def lv_f32(theta, params, seed, pids, it, purpose=1, n_stats=4, paths=False):
    """device_sources/lotka_volterra_f32.hip for the particles `pids` at theta[3, m] (float64): rho[n_stats, m], and with
    paths=True also the emitted outputs [2 n_steps, m] -- operation for operation."""
    theta = np.asarray(theta, dtype=np.float64).reshape(3, -1)
    pids = np.asarray(pids, dtype=np.uint64).reshape(-1)
    m = len(pids)
    n_steps, dt64, sg, x0, y0 = int(params[0]), float(params[1]), float(params[2]), float(params[3]), float(params[4])
    dt, sdt = F(dt64), F(sg * np.sqrt(dt64))
    a, b, c = (theta[j].astype(F) for j in range(3))
    X0, Y0 = F(x0), F(y0)
    X, Y = np.full(m, X0), np.full(m, Y0)
    SX, QX, SY, QY = (np.zeros(m, F) for _ in range(4))
    n_blocks = (n_steps + 1) // 2
    z = box_muller_quad(philox_blocks(seed, pids[:, None], purpose, it, np.arange(n_blocks)[None, :]).reshape(-1, 4)).reshape(m, n_blocks, 4)
    out = np.full((2 * n_steps, m), np.nan)
    for step in range(n_steps):
        z1, z2 = z[:, step // 2, 2 * (step % 2)], z[:, step // 2, 2 * (step % 2) + 1]
        fx = fma32(sdt, z1, fma32(-b, Y, a) * dt)
        fy = fma32(sdt, z2, fma32(b, X, -c) * dt)
        X, Y = np.fmax(fma32(X, fx, X), F(0.0)), np.fmax(fma32(Y, fy, Y), F(0.0))
        dx, dy = X - X0, Y - Y0
        SX, QX, SY, QY = SX + dx, fma32(dx, dx, QX), SY + dy, fma32(dy, dy, QY)
        out[step], out[n_steps + step] = X, Y
    n = float(n_steps)
    stats = []
    for S_, Q_, ref in ((SX, QX, X0), (SY, QY, Y0)):
        S64, Q64 = S_.astype(np.float64), Q_.astype(np.float64)
        md = S64 / n
        with np.errstate(invalid="ignore", over="ignore"):
            v = np.array([R.fma(-s, d, q) if np.isfinite(s) and np.isfinite(d) and np.isfinite(q) else -s * d + q
                          for s, d, q in zip(S64, md, Q64)]) / (n - 1.0)
        stats += [float(ref) + md, np.sqrt(np.fmax(v, 0.0))]
    with np.errstate(invalid="ignore"):
        d = np.abs(np.array(stats)[:n_stats] - np.asarray(params[5:5 + n_stats], dtype=np.float64)[:, None])
        rho = np.where(d < 1e300, d, 1e300)
    return (rho, out) if paths else rho


def fma32_scalar(a, b, c):
    """fma32 for Python floats that hold binary32 values (a per-particle host simulator makes millions of them): the same
    rounding to odd, without NumPy's per-call cost."""
    p = a * b
    s = p + c
    if s - s != 0.0:                                           # inf or NaN
        return float(F(s))
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    if err != 0.0:
        if s != 0.0 and (err < 0.0) == (s > 0.0):
            s = math.nextafter(s, 0.0)
        if not struct.unpack("<q", struct.pack("<d", s))[0] & 1:
            s = math.nextafter(s, math.copysign(math.inf, s))
    return float(F(s))


def lv_f32_one(theta, params, z):
    """lv_f32 for ONE particle from its normals z[n_blocks, 4] (float32), in scalar arithmetic: rho[4]."""
    n_steps, dt64, sg, x0, y0 = int(params[0]), float(params[1]), float(params[2]), float(params[3]), float(params[4])
    f = lambda v: float(F(v))                                  # one rounding to binary32
    dt, sdt = f(dt64), f(sg * math.sqrt(dt64))
    a, b, c = f(theta[0]), f(theta[1]), f(theta[2])
    X0, Y0 = f(x0), f(y0)
    X, Y, SX, QX, SY, QY = X0, Y0, 0.0, 0.0, 0.0, 0.0
    zz = z.astype(np.float64).reshape(-1).tolist()
    for step in range(n_steps):
        z1, z2 = zz[2 * step], zz[2 * step + 1]
        fx = fma32_scalar(sdt, z1, f(fma32_scalar(-b, Y, a) * dt))
        fy = fma32_scalar(sdt, z2, f(fma32_scalar(b, X, -c) * dt))
        X, Y = fma32_scalar(X, fx, X), fma32_scalar(Y, fy, Y)
        X, Y = (X if X > 0.0 else 0.0), (Y if Y > 0.0 else 0.0)          # fmaxf(., 0): a NaN gives 0
        dx, dy = f(X - X0), f(Y - Y0)
        SX, QX, SY, QY = f(SX + dx), fma32_scalar(dx, dx, QX), f(SY + dy), fma32_scalar(dy, dy, QY)
    n = float(n_steps)
    rho = []
    for (S_, Q_, ref), obs in zip(((SX, QX, X0), (SY, QY, Y0)), (params[5:7], params[7:9])):
        md = S_ / n
        finite = math.isfinite(S_) and math.isfinite(Q_)
        v = (R.fma(-S_, md, Q_) if finite else -S_ * md + Q_) / (n - 1.0)
        for st, ob in zip((ref + md, math.sqrt(v) if v > 0.0 else 0.0), obs):     # sqrt(fmax(v, 0)): a NaN gives 0
            d = abs(st - float(ob))
            rho.append(d if d < 1e300 else 1e300)
    return rho


class StreamF32:
    """NormalStream as a source simulator sees it, the binary32 draws included: one block counter for all of them."""

    def __init__(self, O, seed, pid, it, purpose=1):
        self.O, self.seed, self.pid, self.it, self.purpose, self.k = O, seed, pid, it, purpose, 0

    def _blocks(self, n):
        w = blocks(self.O, self.seed, self.pid, self.purpose, self.it, self.k, n)
        self.k += n
        return w

    def quads_f32(self, n):
        """for_quads_f32(n, ...): float32[n, 4]."""
        return box_muller_quad(self._blocks(n)) if n else np.zeros((0, 4), F)

    def quad_f32(self):
        return box_muller_quad(self._blocks(1))[0]

    def uniform_quad_f32(self):
        return uniform_quad(self._blocks(1))[0]

    def normal_pair(self):
        z = self.O.normal_pair(self.seed, self.pid, self.purpose, self.it, self.k)
        self.k += 1
        return z
