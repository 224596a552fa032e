"""The binary32 draws of the device generator (csrc/device_rng.hpp, namespace f32; NormalStream::quad_f32, uniform_quad_f32,
for_quads_f32) on the CPU: their NumPy restatement (tests/elementary_f32_ref.py) against exact arithmetic, its specification,
the distribution of what it draws, the LotkaVolterraF32 simulator over it against an independent f64 Euler-Maruyama, and
that the sources compile and the C symbols exist.  tests/test_gpu_f32_draws.py holds the device to the restatement's bits."""
import ctypes as C

import numpy as np
import pytest

from tests import elementary_f32_ref as E
from tests import elementary_ref as R
from tests.cases import SEED

F = np.float32
# the worst error of a restated normal against mpmath on the same u and angle, in ulps of binary32, measured by
# test_normals_against_exact_arithmetic over its input set: 3.53 (the table sine and cosine bring 2.4 of it, the logarithm 1.2
# halved by the root, the root and the product half an ulp each); asserted: the next half ulp above it (the header comment
# of csrc/device_rng.hpp quotes both)
MAX_ULPS = 4.0

# 8 x quad_f32, 4 x uniform_quad_f32, a for_quads_f32 of 5 blocks, one f64 pair(): 32 + 16 + 20 + 2 = 70 values > 64, so the
# loop's normals are summed per block (5 sums): 32 + 16 + 5 + 2 = 55 values in draw order, the rest zero
PROBE_SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  for (int j = 0; j < 64; ++j) rho[j] = 0.0;
  for (int j = 0; j < 8; ++j) {
    float z0, z1, z2, z3;
    rng.quad_f32(z0, z1, z2, z3);
    rho[4 * j] = (double)z0; rho[4 * j + 1] = (double)z1; rho[4 * j + 2] = (double)z2; rho[4 * j + 3] = (double)z3;
  }
  for (int j = 0; j < 4; ++j) {
    float u0, u1, u2, u3;
    rng.uniform_quad_f32(u0, u1, u2, u3);
    rho[32 + 4 * j] = (double)u0; rho[33 + 4 * j] = (double)u1; rho[34 + 4 * j] = (double)u2; rho[35 + 4 * j] = (double)u3;
  }
  int b = 0;
  rng.for_quads_f32(5, [&](const float z0, const float z1, const float z2, const float z3) {
    rho[48 + b++] = (((double)z0 + (double)z1) + (double)z2) + (double)z3;
  });
  double z0, z1;
  rng.pair(z0, z1);
  rho[53] = z0;
  rho[54] = z1;
}
"""

# n = 1 + (int)theta[0] blocks by for_quads_f32 (theta ~ U(0, 70): 1 .. 70 blocks, straddling 1, W, W + 1, 4 W, 4 W + 1 and
# 4 W + W + 3 for teams of W = 4 and 16), then a quad_f32, then a pair(): the stream must stand at block n, then n + 1
POSITION_SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const int n = 1 + (int)theta[0];
  double acc = 0.0;
  rng.for_quads_f32(n, [&](const float z0, const float z1, const float z2, const float z3) {
    acc += (double)z0; acc += (double)z1; acc += (double)z2; acc += (double)z3;
  });
  float q0, q1, q2, q3;
  rng.quad_f32(q0, q1, q2, q3);
  double z0, z1;
  rng.pair(z0, z1);
  rho[0] = fabs(acc);
  rho[1] = fabs((double)q0);
  rho[2] = fabs(z0);
  rho[3] = fabs(theta[0] - p[0]) + 0.1 * fabs(z1);
}
"""
POSITION_TARGET = 30.0

WIDE_SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  for (int j = 0; j < 48; ++j) rho[j] = 0.0;
  int b = 0;
  rng.for_quads_f32(12, [&](const float z0, const float z1, const float z2, const float z3) {
    rho[4 * b] = fabs(theta[0] + (double)z0); rho[4 * b + 1] = fabs((double)z1); rho[4 * b + 2] = fabs((double)z2);
    rho[4 * b + 3] = fabs((double)z3);
    ++b;
  });
}
"""

LV_OBS = (18.0, 17.0, 14.0, 12.0)


def f64_pair(w):
    """NormalStream::pair() of one block, restated (tests/elementary_ref.py): the device's bits."""
    ua, ub = R.u52(w[0], w[1]), R.u52(w[2], w[3])
    r = R.sqrt_fast(R.neg2_log_tab(ua))
    sn, cs = R.sincos_2pi_tab(ub)
    return r * cs, r * sn


def probe_ref(O, pid, it):
    rng = E.StreamF32(O, SEED, pid, it)
    out = np.zeros(64)
    out[:32] = rng.quads_f32(8).reshape(-1)               # eight single calls are the next eight blocks
    for j in range(4):
        out[32 + 4 * j:36 + 4 * j] = rng.uniform_quad_f32()
    z = rng.quads_f32(5).astype(np.float64)
    out[48:53] = ((z[:, 0] + z[:, 1]) + z[:, 2]) + z[:, 3]
    assert rng.k == 17
    out[53:55] = f64_pair(O.stream_block(SEED, pid, 1, it, rng.k))
    return out


def position_f(O, pid, it, theta):
    th = float(np.atleast_1d(theta)[0])
    rng = E.StreamF32(O, SEED, pid, it)
    n = 1 + int(th)
    acc = 0.0
    for v in rng.quads_f32(n).astype(np.float64).reshape(-1):
        acc += v
    q = rng.quad_f32()
    z0, z1 = rng.normal_pair()
    assert rng.k == n + 2
    return abs(acc), abs(float(q[0])), abs(z0), abs(th - POSITION_TARGET) + 0.1 * abs(z1)


def edge_words():
    """All 2^k and 2^k +- 1, the words around every bin edge of the two tables, and 2e5 random words, as (a, b) pairs."""
    w = {0, 1, 2, 0xFFFFFFFF, 0xFFFFFFFE}
    for k in range(1, 32):
        w |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
    # radius: u = (a + 1/2) 2^-32 crosses a bin edge of the log table where its mantissa's 8th bit flips: around a = (257 + 2 i) 2^e
    for e in (0, 8, 16, 23):
        for i in range(128):
            edge = ((257 + 2 * i) << e) >> 1
            w |= {max(edge - 1, 0), edge, min(edge + 1, 0xFFFFFFFF)}
    # angle: the rows of sct change at odd multiples of 2^26
    for k in range(32):
        edge = (2 * k + 1) << 26
        w |= {edge - 256, edge - 1, edge, edge + 255, edge + 256}
    w = np.array(sorted(w), dtype=np.uint32)
    rng = np.random.default_rng(SEED)
    a = np.concatenate([w, rng.permutation(w), rng.integers(0, 1 << 32, 200_000, dtype=np.uint64).astype(np.uint32)])
    b = np.concatenate([w, w, rng.integers(0, 1 << 32, 200_000, dtype=np.uint64).astype(np.uint32)])
    return a, b


def test_the_vectorised_fma_rounds_once():
    """Against exact rationals: random operands with cancellation, and the midpoint cases a product + sum in binary64 gets
    wrong -- c + a b with a b = 2^-16 (1 - 2^-46) half an ulp of c = 256 (1 + k 2^-23) less 2^-62: binary64 rounds the sum to
    the midpoint itself, and a second rounding to even then goes up for odd k, where the exact sum lies below the midpoint."""
    rng = np.random.default_rng(1)
    a = rng.standard_normal(2000).astype(F)
    b = rng.standard_normal(2000).astype(F)
    c = (-(a.astype(np.float64) * b) * (1.0 + rng.standard_normal(2000) * 1e-7)).astype(F)
    a2 = np.full(1000, F(1.0) + F(2.0 ** -23))
    b2 = np.full(1000, (F(1.0) - F(2.0 ** -23)) * F(2.0 ** -16))
    c2 = (256.0 * (1.0 + rng.integers(0, 1 << 23, 1000) * 2.0 ** -23)).astype(F)
    a, b, c = np.concatenate([a, a2, a2]), np.concatenate([b, b2, -b2]), np.concatenate([c, c2, c2])
    want = np.array([E.fma32_exact(x, y, z) for x, y, z in zip(a, b, c)], dtype=F)
    got = E.fma32(a, b, c)
    naive = (a.astype(np.float64) * b + c).astype(F)
    assert (naive.view(np.uint32) != want.view(np.uint32)).sum() > 100, "the midpoint cases do not bite: the check is empty"
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_the_numpy_philox_is_the_oracles(O):
    pids = np.array([0, 77, (1 << 33) + 12345], dtype=np.uint64)
    for purpose, it in ((1, 3), (6, (5 << 32) + 900)):
        got = E.philox_blocks(SEED, pids[:, None], purpose, it, np.arange(4)[None, :])
        want = np.array([[O.stream_block(SEED, int(p), purpose, it, k) for k in range(4)] for p in pids], dtype=np.uint32)
        np.testing.assert_array_equal(got, want)


def test_normals_against_exact_arithmetic():
    import mpmath
    mp = mpmath.mp.clone()
    mp.prec = 100
    a, b = edge_words()
    z0, z1 = E.pair(a, b)
    u = E.radius_uniform(a)
    two_pi = 2 * mp.pi
    worst, where = 0.0, None
    for i in range(len(a)):
        ang = two_pi * mp.mpf(int(b[i]) >> 8) / (1 << 24)
        rad = mp.sqrt(-2 * mp.log(mp.mpf(float(u[i]))))
        quarter = (int(b[i]) >> 8) % (1 << 22) == 0           # a multiple of a quarter turn: sin or cos is 0 exactly
        for got, ex, zero in ((z0[i], rad * mp.cos(ang), quarter and (int(b[i]) >> 30) % 2 == 1),
                              (z1[i], rad * mp.sin(ang), quarter and (int(b[i]) >> 30) % 2 == 0)):
            if zero or rad == 0:
                assert abs(float(got)) <= 1e-6 * float(rad), (hex(a[i]), hex(b[i]), got)      # the table's cos(pi/2) is 6e-17, not 0
                continue
            exf = float(ex)
            err = abs(float(mp.mpf(float(got)) - ex)) / float(np.spacing(F(abs(exf))))
            if err > worst:
                worst, where = err, (hex(a[i]), hex(b[i]), float(got), exf)
    print(f"binary32 normals against mpmath on the same u and angle, {2 * len(a)} values: worst {worst:.3f} ulp at {where}")
    assert worst <= MAX_ULPS


def test_specification_of_the_block():
    """u == 1 gives z == 0 exactly, never a NaN; max |z| is the documented bound sqrt(66 ln 2); the uniforms lie in (0, 1) and
    are exact."""
    top = np.array([0xFFFFFFFF, 0xFFFFFF80, 0xFFFFFF7F], dtype=np.uint32)       # (float)a = 2^32 from 0xFFFFFF80 on
    assert list(E.radius_uniform(top)) == [1.0, 1.0, F(1.0) - F(2.0 ** -24)]
    angles = np.array([0, 5, 1 << 30, 0xDEADBEEF], dtype=np.uint32)
    for a in top[:2]:
        z0, z1 = E.pair(np.full(4, a, np.uint32), angles)
        assert np.all(z0 == 0.0) and np.all(z1 == 0.0)
    z0, z1 = E.pair(np.zeros(2, np.uint32), np.array([0, 1 << 31], np.uint32))  # u = 2^-33 at angles 0 and pi
    assert float(z0[0]) == float(F(E.Z_MAX)) == -float(z0[1]) and abs(E.Z_MAX - 6.7637) < 1e-4
    rng = np.random.default_rng(SEED)
    a, b = edge_words()
    z = np.concatenate(E.pair(a, b))
    assert np.all(np.isfinite(z)) and np.abs(z).max() <= float(F(E.Z_MAX))
    w = np.concatenate([np.array([0, 0x1FF, 0x200, 0xFFFFFFFF, 0xFFFFFE00], dtype=np.uint32),
                        rng.integers(0, 1 << 32, 99_999, dtype=np.uint64).astype(np.uint32)]).reshape(-1, 4)
    uq = E.uniform_quad(w)
    assert uq.dtype == F and uq.min() == F(2.0 ** -24) and uq.max() == F(1.0) - F(2.0 ** -24)
    np.testing.assert_array_equal(uq.astype(np.float64), ((w >> 9).astype(np.float64) + 0.5) * 2.0 ** -23)


def test_distribution_of_the_restated_normals(O):
    from scipy import stats
    n_blocks = 100_000
    w = np.concatenate([E.blocks(O, SEED, pid, 1, 2, 0, n_blocks // 4) for pid in range(4)])
    assert w.shape == (n_blocks, 4)
    z = E.box_muller_quad(w).astype(np.float64)
    flat = z.reshape(-1)
    n = len(flat)
    p_ks = stats.kstest(flat, "norm").pvalue
    # mean, variance, fourth moment: z-scores under N(0, 1) (variances 1/n, 2/n, 96/n)
    zs = {"mean": flat.mean() * np.sqrt(n), "variance": (np.mean(flat ** 2) - 1.0) * np.sqrt(n / 2.0),
          "fourth moment": (np.mean(flat ** 4) - 3.0) * np.sqrt(n / 96.0)}
    ps = {"KS": p_ks, **{k: float(2 * stats.norm.sf(abs(v))) for k, v in zs.items()}}
    for i in range(4):
        for j in range(i + 1, 4):
            r = np.corrcoef(z[:, i], z[:, j])[0, 1]
            ps[f"corr(z{i}, z{j})"] = float(2 * stats.norm.sf(abs(r) * np.sqrt(n_blocks)))
    per_stream = z.reshape(4, n_blocks // 4, 4)
    lag = np.mean([np.corrcoef(s[:-1].reshape(-1), s[1:].reshape(-1))[0, 1] for s in per_stream])
    ps["lag-1 across blocks"] = float(2 * stats.norm.sf(abs(lag) * np.sqrt(n - 16)))
    print(", ".join(f"{k}: p = {v:.4f}" for k, v in ps.items()))
    for k, v in ps.items():
        assert v > 1e-4, k


def test_lv_restatement_follows_an_independent_f64_euler_maruyama():
    from scipy import stats
    from tests.independent.models_numpy import cfg5
    runs, theta = 4000, np.array([1.0, 0.02, 1.0])
    params = [256, 0.05, 0.1, 50.0, 50.0, *LV_OBS]
    ours = E.lv_f32(np.repeat(theta[:, None], runs, axis=1), params, SEED + 3, np.arange(runs), 2).T
    theirs = cfg5(obs=LV_OBS)["sim"](np.repeat(theta[None, :], runs, axis=0), np.random.default_rng(99))
    assert ours.shape == theirs.shape == (runs, 4) and np.all(ours < 1e29)
    for j, name in enumerate(("mean X", "sd X", "mean Y", "sd Y")):
        p = stats.ks_2samp(ours[:, j], theirs[:, j]).pvalue
        print(f"{name}: two-sample KS p = {p:.4f}")
        assert p > 1e-4, name


def test_lv_sums_of_deviations_keep_their_digits():
    """The running sums in binary32 against the same paths summed in float64: the statistics agree to 1e-5 relatively (sums of
    the states themselves, of the order of 256 x 50^2, would keep three digits of the variance)."""
    params = [256, 0.05, 0.1, 50.0, 50.0, 0.0, 0.0, 0.0, 0.0]
    theta = np.array([[1.0, 0.5], [0.02, 0.03], [1.0, 0.7]])
    rho, out = E.lv_f32(theta, params, SEED, [3, 4], 1, paths=True)
    X, Y = out[:256], out[256:]
    want = np.stack([X.mean(0), X.std(0, ddof=1), Y.mean(0), Y.std(0, ddof=1)])
    np.testing.assert_allclose(rho, want, rtol=1e-5)


def test_the_scalar_lv_restatement_is_the_vectorised_one():
    """tests/test_gpu_f32_draws.py hands the oracle a per-particle host simulator: the scalar spelling, same bits."""
    rng = np.random.default_rng(7)
    for n_steps in (15, 256):
        params = [n_steps, 0.05, 0.1, 50.0, 50.0, *LV_OBS]
        theta = rng.uniform(0.0, 1.0, (3, 40)) * np.array([[2.0], [0.1], [2.0]])
        theta[:, 0] = (2.0, 0.1, 0.0)                                       # a path that blows up
        pids = np.arange(100, 140)
        want = E.lv_f32(theta, params, SEED, pids, 9)
        n_blocks = (n_steps + 1) // 2
        z = E.box_muller_quad(E.philox_blocks(SEED, pids[:, None], 1, 9, np.arange(n_blocks)[None, :]).reshape(-1, 4)).reshape(40, n_blocks, 4)
        got = np.array([E.lv_f32_one(theta[:, i], params, z[i]) for i in range(40)]).T
        np.testing.assert_array_equal(got, want)
    a, b, c = np.float32(1.0) + np.float32(2.0 ** -23), (np.float32(1.0) - np.float32(2.0 ** -23)) * np.float32(2.0 ** -16), np.float32(256.0 + 3 * 2.0 ** -15)
    assert E.fma32_scalar(float(a), float(b), float(c)) == float(E.fma32_exact(a, b, c)) != float(np.float32(float(a) * float(b) + float(c)))


def test_the_sources_compile_without_a_device(S):
    assert S.DeviceSource(PROBE_SRC, 1, 64, []).compile_check()
    assert S.DeviceSource(POSITION_SRC, 1, 4, [POSITION_TARGET]).compile_check()
    assert S.DeviceSource(WIDE_SRC, 1, 48, []).compile_check()                  # the wide form of the kernels
    for n_stats in (4, 1):
        model = S.LotkaVolterraF32(obs=LV_OBS, n_stats=n_stats)
        assert model.n_para == (3,) and model.n_stats == n_stats and model.n_outputs == 512
        assert model.params == [256.0, 0.05, 0.1, 50.0, 50.0, *LV_OBS]
        assert f"#define LV_N_STATS {n_stats}\n" in model.source
    assert S.LotkaVolterraF32(obs=LV_OBS).compile_check()
    import sabc_amd
    assert sabc_amd.LotkaVolterraF32 is S.LotkaVolterraF32
    for bad in (dict(n_steps=1), dict(n_stats=5), dict(obs=(1.0, 2.0))):
        with pytest.raises(ValueError):
            S.LotkaVolterraF32(**bad)


def test_the_new_symbols_exist_and_a_library_without_a_device_says_so(S):
    from tests import cpu_engine
    product, harness = S.lib(), cpu_engine.lib()
    for L in (product, harness):
        assert hasattr(L, "sabc_op_normal_quads_f32") and hasattr(L, "sabc_op_rng_peak_f32")
    assert product.sabc_abi_version() == harness.sabc_abi_version() == 6
    NO_DEVICE = -20
    out, rate = (C.c_float * 8)(), C.c_double()
    quads = harness.sabc_op_normal_quads_f32
    quads.argtypes = [C.c_int32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int64, C.POINTER(C.c_float)]
    peak = harness.sabc_op_rng_peak_f32
    peak.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
    assert quads(0, SEED, 0, 1, 0, 0, 2, out) == NO_DEVICE
    assert peak(0, 64, 1, 1, C.byref(rate)) == NO_DEVICE
    harness.sabc_last_global_error.restype = C.c_char_p
    assert b"no device" in harness.sabc_last_global_error()
