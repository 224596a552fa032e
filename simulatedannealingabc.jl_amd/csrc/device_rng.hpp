// device_rng.hpp -- counter-based Philox4x32-10 per wavefront lane, 52-bit uniforms and
// Box-Muller pairs in f64 for gfx950.  Replaces every rand()/randn() site of the reference
// (SimulatedAnnealingABC.jl:163,174,324; proposals.jl:42,54,105-106,110,141,144).
//
// Stream layout (DESIGN.md "RNG streams"): key = seed; counter = (particle id, block index,
// iteration, purpose).  One block = 128 bits = two 52-bit uniforms = one Box-Muller pair.
// Keyed by GLOBAL particle id, so a run does not depend on how particles are sharded.
#pragma once
#if !defined(__HIPCC_RTC__)     // hipRTC pre-includes the HIP runtime
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#ifndef INFINITY                 // hipRTC has no <math.h>
#define INFINITY (__builtin_huge_val())
#endif
#include "sort_network.hpp"      // sabc::sort_ascending / order_statistic / quantile: part of what a simulator from source sees

namespace sabc {

enum : uint32_t { PURPOSE_PRIOR = 0, PURPOSE_SIM = 1, PURPOSE_PROP = 2, PURPOSE_PROP2 = 3, PURPOSE_ACCEPT = 4,
                  PURPOSE_RESAMPLE = 5,
                  PURPOSE_PREDICT = 6 };   // forward runs for predictive checks (sabc_op_simulate_outputs): streams no update uses

struct u32x4 { uint32_t x, y, z, w; };

// a ^ b ^ c: one v_bitop3_b32 (truth table 0x96, new on gfx950) where the compiler in use knows the builtin -- hipcc of
// ROCm 7.x does; a hipRTC whose clang is older (the GPU box's run-time compiler once lacked a builtin hipcc had) falls
// back to two v_xor_b32.  Same bits either way (the Random123 known answers run through both, tests/test_user_simulator.py).
#if defined(__has_builtin)
#if __has_builtin(__builtin_amdgcn_bitop3_b32) && !defined(SABC_NO_BITOP3)
#define SABC_HAVE_BITOP3 1
#endif
#endif
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(SABC_HAVE_BITOP3)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
  return a ^ b ^ c;
#endif
}

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2,
                                               uint32_t c3) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // one v_mad_u64_u32 per product: hi and lo halves come from the same instruction
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    // three-input XOR in one instruction where available (xor3)
    const uint32_t n0 = xor3((uint32_t)(p1 >> 32), c1, k0);
    const uint32_t n2 = xor3((uint32_t)(p0 >> 32), c3, k1);
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return u32x4{c0, c1, c2, c3};
}

__device__ __forceinline__ u32x4 stream_block(uint64_t seed, uint64_t pid, uint32_t purpose, uint64_t iter,
                                              uint32_t k) {
  const uint32_t c3 = (purpose & 0xFFu) | ((uint32_t)(pid >> 32) << 8) | ((uint32_t)((iter >> 32) & 0xFFu) << 24);
  return philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)pid, k, (uint32_t)iter, c3);
}

// (x + 1/2) * 2^-52 with x = (low 20 bits of hi):(all of lo): exact in binary64, in (0,1).
// Built without a shift or an int->fp conversion: those 52 bits ARE the mantissa of a double in [1,2)
// (a v_and_b32 and a v_or_b32 on the high word: a gfx9 VOP3 instruction takes ONE literal, and 0xFFFFF and 0x3FF00000 are
// two; loop::u52 below, with the exponent word in a register, is the one v_and_or_b32), and (1 - 2^-53) is subtracted, which is exact.
__device__ __forceinline__ double u52(uint32_t hi, uint32_t lo) {
  const double d = __hiloint2double((int)(0x3FF00000u | (hi & 0xFFFFFu)), (int)lo);
  return d - 0x1.fffffffffffffp-1;
}

__device__ __forceinline__ uint64_t pack64(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | lo; }

// ---- f64 elementary functions specialised to the Box-Muller input ranges -------------------
// ocml's log / sincospi / sqrt are correctly-rounded-grade general routines built on double-double
// arithmetic (52 v_add_f64 per pair in the ISA).  The inputs here are known: u in [2^-53, 1), so
// no special values, no denormals, no range reduction beyond one table-free step.  Worst errors against exact arithmetic, in
// ulps of the exact result, measured and asserted by tests/test_elementary_functions.py (on the device unless marked):
// div_fast, sqrt_fast correctly rounded at every point tested (asserted: 1 ulp); log_fast 0.73 (1); neg2_log_tab 1.87 on (0, 1),
// 1.58 above 1 (2, restated on the CPU; the device gives the restatement's bits, as for sincos_2pi_tab and exp_tab);
// exp_tab 1.79 (2); log_factorial 1.70 (2); absolutely, in units of 2^-53: sincos_2pi_tab 1.12 (1.25), tanh_abs_tab 2.56 (3.06).

// q = a / b for finite, normal a, b of moderate magnitude: v_rcp_f64 + two Newton steps + one
// residual correction (what the compiler emits for '/', minus the scale/fixup for special values)
__device__ __forceinline__ double div_fast(double a, double b) {
  double r = __builtin_amdgcn_rcp(b);
  r = fma(fma(-b, r, 1.0), r, r);
  r = fma(fma(-b, r, 1.0), r, r);
  const double q = a * r;
  return fma(fma(-b, q, a), r, q);
}

// sqrt(x) for x in [1e-300, 1e300]: v_rsq_f64 (~2^-27), one coupled Newton step, one residual correction
// (what the compiler emits for sqrt(), minus its second correction and the scaling for tiny / huge x)
__device__ __forceinline__ double sqrt_fast(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = 0.5 * y;
  const double r = fma(-h, g, 0.5);
  g = fma(g, r, g); h = fma(h, r, h);
  return fma(fma(-g, g, x), h, g);
}

// log(x) for normal x > 0: x = 2^e m with m in [sqrt(1/2), sqrt(2)), log m = 2 atanh(s),
// s = (m-1)/(m+1), degree-7 minimax polynomial in s^2 (the classic fdlibm scheme and constants)
__device__ __forceinline__ double log_fast(double x) {
  const uint64_t ix = (uint64_t)__double_as_longlong(x);
  int hx = (int)(ix >> 32);
  hx += 0x3ff00000 - 0x3fe6a09e;
  const int e = (hx >> 20) - 0x3ff;
  hx = (hx & 0x000fffff) + 0x3fe6a09e;
  const double m = __longlong_as_double((long long)(((uint64_t)(uint32_t)hx << 32) | (ix & 0xffffffffull)));
  const double f = m - 1.0;
  const double hfsq = 0.5 * f * f;
  const double s = div_fast(f, 2.0 + f);
  const double z = s * s, w = z * z;
  const double t1 = w * fma(w, fma(w, 1.531383769920937332e-01, 2.222219843214978396e-01), 3.999999999940941908e-01);
  const double t2 = z * fma(w, fma(w, fma(w, 1.479819860511658591e-01, 1.818357216161805012e-01),
                                   2.857142874366239149e-01), 6.666666666666735130e-01);
  const double R = t2 + t1;
  const double dk = (double)e;
  return fma(dk, 6.93147180369123816490e-01, (fma(s, hfsq + R, dk * 1.90821492927058770002e-10) - hfsq) + f);
}

// ---- table-driven log and sin/cos for the Box-Muller pair ------------------------------------
// The pair costs one log and one sin/cos; with two small tables in LDS (2.5 KB, rng_tables.inc, generated by
// tools/gen_rng_tables.py) both shrink to short polynomials on a tiny argument: log 33 -> 19 VALU instructions
// (no division), sin/cos 34 -> 23 (no quadrant selects).  Every kernel that draws normals calls
// rng_tables_init() first (all threads of the workgroup, before any divergent return).
#include "rng_tables.inc"

struct RngTables {
  double2 logt[128];     // -2 x { 1/c_i rounded, -log of that }: c_i = 1 + i/128 (i < 53) or (1 + i/128)/2 (i >= 53); c_0 = 1
  double2 sct[33];       // { sin, cos } of 2 pi k / 32, k = 0..32 (row 32 = row 0)
  double exp2t[32];      // 2^(j/32)
};

__device__ __forceinline__ RngTables &rng_tables() {
  __shared__ RngTables t;
  return t;
}

// the copies only; the caller's next __syncthreads() publishes them (k_update shares that barrier with its ECDF index)
__device__ __forceinline__ void rng_tables_load() {
  RngTables &t = rng_tables();
  const int i = threadIdx.x;
  if (blockDim.x >= 128) {
    // every table entry has a thread of its own: the three reads go out together and the workgroup starts after ONE trip
    // to memory (three loops, each waiting for its own read, were three -- at the front of every workgroup's life)
    double2 a = make_double2(0.0, 0.0), b = make_double2(0.0, 0.0);
    double c = 0.0;
    if (i < 128) a = make_double2(kLogTab[i][0], kLogTab[i][1]);
    if (i < 33) b = make_double2(kSinCosTab[i & 31][0], kSinCosTab[i & 31][1]);
    if (i < 32) c = kExp2Tab[i];
    if (i < 128) t.logt[i] = a;
    if (i < 33) t.sct[i] = b;
    if (i < 32) t.exp2t[i] = c;
    return;
  }
  for (int k = i; k < 128; k += blockDim.x) t.logt[k] = make_double2(kLogTab[k][0], kLogTab[k][1]);
  for (int k = i; k < 33; k += blockDim.x) t.sct[k] = make_double2(kSinCosTab[k & 31][0], kSinCosTab[k & 31][1]);
  for (int k = i; k < 32; k += blockDim.x) t.exp2t[k] = kExp2Tab[k];
}

__device__ __forceinline__ void rng_tables_init() {
  rng_tables_load();
  __syncthreads();
}

// -2 log(x), normal x > 0 (the squared Box-Muller radius).  x = 2^E m; the 7 leading mantissa bits (rounded to
// nearest, so that 1 is a bin CENTRE) pick c_i with |m / c_i - 1| <= 2^-8; bins above sqrt(2) are taken as c_i / 2
// with E + 1, so m / c stays in [0.707, 1.414) and there is no cancellation against E ln 2 for x near 1 (x -> 1
// from below lands in bin 0 of E = 0: c = 1, full relative accuracy).  log(m) = logc_i + log1p(r), r = m inv_i - 1.
// With s = -2 r (one fma against the table's -2 inv_i): -2 log1p(r) = s + s^2/4 + s^3/12 + ... + s^7/448
// (remainder 2^-59 relative on |s| <= 2^-7; half a bin is 1 << 12 of the high word -- with less added, 1 is no centre, |s|
// reaches 1.5 x 2^-7 and bin 127's entry cancels against the polynomial just below 1: 3.9 ulp there against 1.87).
__device__ __forceinline__ double neg2_log_tab(double x) {
  const uint32_t hi = (uint32_t)__double2hiint(x);
  const uint32_t t = hi + 0x1000u;                      // round the mantissa to 7 bits (may carry into the exponent)
  const uint32_t tp = t + (75u << 13);                  // ... and carry when that rounded mantissa is >= 53/128
  const int nE = 1023 - (int)(tp >> 20);                // -E
  const double m = __hiloint2double((int)(hi + ((uint32_t)nE << 20)), __double2loint(x));   // x 2^-E, exact
  const double2 e = rng_tables().logt[(t >> 13) & 127u];
  const double s = fma(m, e.x, 2.0);                    // -2 (m inv - 1)
  double p = 1.0 / 448.0;
  p = fma(p, s, 1.0 / 192.0);
  p = fma(p, s, 1.0 / 80.0);
  p = fma(p, s, 1.0 / 32.0);
  p = fma(p, s, 1.0 / 12.0);
  p = fma(p, s, 0.25);
  const double l = fma(s * s, p, s);
  const double nEd = (double)nE;
  // the product and the polynomial have the same sign (both >= 0 for x < 1, both <= 0 for x > 1) and the table entry is
  // small, so one rounded product is accurate to about half an ulp of the sum: no hi/lo split of ln 2 needed
  return fma(nEd, 2.0 * 6.93147180559945309417e-01, e.y) + l;
}

// sin and cos of 2 pi u, u in (0,1): k = rint(32 u), f = 32 u - k exact, r = (pi/16) f, |r| <= pi/32;
// sin(a_k + r) = S + (S q + C sin r), cos(a_k + r) = C + (C q - S sin r) with q = cos r - 1 and (S, C) from the table.
__device__ __forceinline__ void sincos_2pi_tab(double u, double &sn, double &cs) {
  // k = rint(32 u) by the add-a-big-number trick: the sum's low mantissa word IS k (0..32; the table has 33 rows),
  // which saves the conversion and the wrap-around mask
  const double tm = fma(u, 32.0, 0x1.8p52);
  const double kf = tm - 0x1.8p52;
  const double r = 1.96349540849362077404e-01 * fma(u, 32.0, -kf);       // (pi / 16) (32 u - k), the difference is exact
  const double2 sc = rng_tables().sct[__double2loint(tm)];
  const double r2 = r * r;
  double p = 1.0 / 362880.0;
  p = fma(p, r2, -1.0 / 5040.0);
  p = fma(p, r2, 1.0 / 120.0);
  p = fma(p, r2, -1.0 / 6.0);
  const double sr = fma(r * r2, p, r);                                    // sin r
  double q = 1.0 / 40320.0;
  q = fma(q, r2, -1.0 / 720.0);
  q = fma(q, r2, 1.0 / 24.0);
  q = fma(q, r2, -0.5);
  q *= r2;                                                                // cos r - 1
  sn = sc.x + fma(sc.x, q, sc.y * sr);
  cs = sc.y + fma(sc.y, q, -(sc.x * sr));
}

// exp(x), |x| <= 700 (clamped): x = (32 e + j) ln2/32 + r with |r| <= ln2/64, exp(x) = 2^e 2^(j/32) exp(r); the integer
// 32 e + j by the add-a-big-number trick (two's complement in the sum's low word), 2^(j/32) from the table, exp(r) by
// its Taylor polynomial of degree 6 (remainder 4e-18).  15 VALU instructions against 21 for a table-free version with a degree-13 polynomial, and 7 polynomial
// constants instead of 13 (the g-and-k kernel, which calls it four times per draw pair, is short of scalar registers).
// HI = 700: the clamp of every caller but one.  HI = 710 (gk_quantile, device_models.hpp): the same steps carry on to the end
// of the doubles -- e = 1024 is +inf out of ldexp, so exp(x) = +inf from x = 709.79 on, as the definition has it, and the
// values below 700 are the same bits.
template <int HI>
__device__ __forceinline__ double exp_tab_upto(double x) {
  static_assert(HI == 700 || HI == 710, "the reduction is exact for |32 x / ln 2| < 2^31; 2^(j/32) exp(r) >= 1 makes e = 1024 +inf");
  x = fmin(fmax(x, -700.0), (double)HI);
  const double tm = fma(x, 0x1.71547652b82fep+5, 0x1.8p52);             // 32 / ln 2
  const double nf = tm - 0x1.8p52;
  const int n = __double2loint(tm);
  double r = fma(-nf, 0x1.62e42feep-6, x);                                // ln2/32, 32 significant bits: exact product
  r = fma(-nf, 0x1.a39ef35793c76p-38, r);
  const double t = rng_tables().exp2t[n & 31];
  double p = 1.0 / 720.0;
  p = fma(p, r, 1.0 / 120.0);
  p = fma(p, r, 1.0 / 24.0);
  p = fma(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(t * p, n >> 5);
}
__device__ __forceinline__ double exp_tab(double x) { return exp_tab_upto<700>(x); }

// tanh(y) = sign(y) (1 - 2 / (exp(2|y|) + 1)): absolute error 2.56 x 2^-53 = 2.8e-16 (the relative error near 0 is not controlled,
// which is fine where it is used: inside 1 + c tanh(.))
__device__ __forceinline__ double tanh_abs_tab(double y) {
  const double a = fmin(fabs(y), 20.0);
  const double t = 1.0 - div_fast(2.0, exp_tab(2.0 * a) + 1.0);
  return copysign(t, y);
}

// log(k!) = lgamma(k + 1) for an integer-valued k >= 0 (the count draws' acceptance tests; the library's lgamma is a long general
// routine): k < 16 from a table, else Stirling's series in x = k + 1 >= 17 through 1/(1188 x^9) -- the first term left out is
// below 6e-17 absolutely, so the error is that of (x - 1/2) log x: 1.70 ulp of the result at the worst (k <= 2^30)
static __device__ const double kLogFactorial[16] = {0.0, 0.0, 0.6931471805599453, 1.791759469228055, 3.1780538303479458, 4.787491742782046, 6.579251212010101, 8.525161361065415, 10.60460290274525, 12.801827480081469, 15.104412573075516, 17.502307845873887, 19.987214495661885, 22.552163853123425, 25.19122118273868, 27.89927138384089};
__device__ __forceinline__ double log_factorial(const double k) {
  if (k < 16.0) return kLogFactorial[(int)k];
  const double x = k + 1.0, r = div_fast(1.0, x), r2 = r * r;
  double p = 1.0 / 1188.0;
  p = fma(p, r2, -1.0 / 1680.0);
  p = fma(p, r2, 1.0 / 1260.0);
  p = fma(p, r2, -1.0 / 360.0);
  p = fma(p, r2, 1.0 / 12.0);
  return fma(x - 0.5, log_fast(x), -x) + fma(p, r, 9.18938533204672741780e-01);      // + log(2 pi) / 2
}

__device__ __forceinline__ void box_muller(const u32x4 w, double &z0, double &z1) {
  const double ua = u52(w.x, w.y);
  const double ub = u52(w.z, w.w);
  const double r = sqrt_fast(neg2_log_tab(ua));
  double sn, cs;
  sincos_2pi_tab(ub, sn, cs);
  z0 = r * cs;
  z1 = r * sn;
}

// ---- the same generator, re-spelled for the simulators' loop (NormalStream::for_pairs with a lane per particle) --------------
// The update kernels sit at the VALU issue ceiling and nine tenths of their instructions come from that loop, so it is worth
// spelling it for the instruction count: 94 -> 85 VALU instructions per pair (tests/test_generator_isa.py).  Nothing here
// changes arithmetic -- same words, same products, same FMAs in the same order (tests/test_generator_bits.py holds the bits
// against the build before) --, and the functions above stay as they are for every other draw: a re-spelled one-off draw gains
// nothing and shifts the register allocation of kernels that sit on their register cap.
namespace loop {

// Philox with the wave-uniform half of rounds 1-2 on the scalar unit.  In the streams' layout (stream_block) c1, c2, c3 and the
// key are the same on every lane of a wave, only c0 = the particle id differs: round 1's M1 c2 and n0 and round 2's M0 c0 are
// uniform.  xor3's builtin is a VALU instruction whatever its operands are and pins them (and the two multiplies behind) to
// the VALU; the plain XOR leaves them to the scalar unit (s_xor_b32, s_mul_i32, s_mul_hi_u32), idle in this loop.  Rounds 3-10
// keep the three-input XOR (the compiler does not form it by itself).
__device__ __forceinline__ u32x4 philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = r < 2 ? (uint32_t)(p1 >> 32) ^ c1 ^ k0 : xor3((uint32_t)(p1 >> 32), c1, k0);
    const uint32_t n2 = r < 2 ? (uint32_t)(p0 >> 32) ^ c3 ^ k1 : xor3((uint32_t)(p0 >> 32), c3, k1);
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return u32x4{c0, c1, c2, c3};
}

__device__ __forceinline__ u32x4 stream_block(uint64_t seed, uint64_t pid, uint32_t purpose, uint64_t iter, uint32_t k) {
  const uint32_t c3 = (purpose & 0xFFu) | ((uint32_t)(pid >> 32) << 8) | ((uint32_t)((iter >> 32) & 0xFFu) << 24);
  return loop::philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)pid, k, (uint32_t)iter, c3);
}

// The constants of a pair that the instruction set cannot take as immediates where they are used, held in registers that the
// compiler has to treat as unknown values, so that it cannot rebuild them in front of every use (v_mov_b32: four per pair).
// Loaded ONCE in front of the loop.
struct Regs {
  uint32_t one_hi;     // 0x3FF00000, the high word of 1.0, in a vector register: u52 is one v_and_or_b32
  double big;          // 0x1.8p52, sincos_2pi_tab's add-a-big-number constant, in a vector register pair ...
  double k32;          // ... and 32.0 in a scalar pair: fma(u, 32, big) is the three-address v_fma_f64 that reads big where it
                       // is (with 32.0 as a literal it is the two-address v_fmac_f64 on a copy of big)
  __device__ __forceinline__ static Regs load() {
    Regs r{0x3FF00000u, 0x1.8p52, 32.0};
    asm("" : "+v"(r.one_hi));
    asm("" : "+v"(r.big));
    asm("" : "+s"(r.k32));
    return r;
  }
};

__device__ __forceinline__ double u52(uint32_t hi, uint32_t lo, const Regs &c) {
  const double d = __hiloint2double((int)(c.one_hi | (hi & 0xFFFFFu)), (int)lo);
  return d - 0x1.fffffffffffffp-1;
}

// neg2_log_tab with the power of two in the TABLE ENTRY's exponent, not in x's: s = m (-2 inv) + 2 with m = x 2^-E is also
// x (2^-E (-2 inv)) + 2.  Both scalings are exact and the two products are the same real number, so the fma rounds to the same
// s; but a new high word on x costs a copy of its low word (the pair x lives in is still read), on the loaded entry it does not.
// (x in [2^-1000, 2^1000]: the entry's exponent must stay in range.  Box-Muller's x is in (0, 1).)
__device__ __forceinline__ double neg2_log_tab(double x) {
  const uint32_t hi = (uint32_t)__double2hiint(x);
  const uint32_t t = hi + 0x1000u;
  const uint32_t tp = t + (75u << 13);
  const int nE = 1023 - (int)(tp >> 20);
  const double2 e = rng_tables().logt[(t >> 13) & 127u];
  const double ex = __hiloint2double((int)((uint32_t)__double2hiint(e.x) + ((uint32_t)nE << 20)), __double2loint(e.x));
  const double s = fma(x, ex, 2.0);
  double p = 1.0 / 448.0;
  p = fma(p, s, 1.0 / 192.0);
  p = fma(p, s, 1.0 / 80.0);
  p = fma(p, s, 1.0 / 32.0);
  p = fma(p, s, 1.0 / 12.0);
  p = fma(p, s, 0.25);
  const double l = fma(s * s, p, s);
  const double nEd = (double)nE;
  return fma(nEd, 2.0 * 6.93147180559945309417e-01, e.y) + l;
}

__device__ __forceinline__ void sincos_2pi_tab(double u, double &sn, double &cs, const Regs &c) {
  const double tm = fma(u, c.k32, c.big);
  const double kf = tm - c.big;
  const double r = 1.96349540849362077404e-01 * fma(u, 32.0, -kf);
  const double2 sc = rng_tables().sct[__double2loint(tm)];
  const double r2 = r * r;
  double p = 1.0 / 362880.0;
  p = fma(p, r2, -1.0 / 5040.0);
  p = fma(p, r2, 1.0 / 120.0);
  p = fma(p, r2, -1.0 / 6.0);
  const double sr = fma(r * r2, p, r);
  double q = 1.0 / 40320.0;
  q = fma(q, r2, -1.0 / 720.0);
  q = fma(q, r2, 1.0 / 24.0);
  q = fma(q, r2, -0.5);
  q *= r2;
  sn = sc.x + fma(sc.x, q, sc.y * sr);
  cs = sc.y + fma(sc.y, q, -(sc.x * sr));
}

__device__ __forceinline__ void box_muller(const u32x4 w, double &z0, double &z1, const Regs &c) {
  const double ua = loop::u52(w.x, w.y, c);
  const double ub = loop::u52(w.z, w.w, c);
  const double r = sqrt_fast(loop::neg2_log_tab(ua));
  double sn, cs;
  loop::sincos_2pi_tab(ub, sn, cs, c);
  z0 = r * cs;
  z1 = r * sn;
}

}  // namespace loop

// A TEAM of W = 4 or 16 lanes (a quad | a row of the wave) that run one particle side by side: the value lane (team base + J)
// holds, on every lane of the team -- one DPP move per 32-bit half, no LDS (quad_perm [J, J, J, J] | row_newbcast:J).
template <int W, int J>
__device__ __forceinline__ double team_pick_ct(const double v) {
  static_assert((W == 4 || W == 16) && J >= 0 && J < W, "a quad or a row of 16 lanes");
  constexpr int ctrl = W == 4 ? J * 0x55 : 0x150 + J;
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), ctrl, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), ctrl, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// ---- f32 draws: four N(0,1) per Philox block (NormalStream::quad_f32 / for_quads_f32) -------------------------------------
// A block w = (x, y, z, w) gives (z0, z1) from (x, y) and (z2, z3) from (z, w).  Of a pair (a, b):
//   radius uniform  u = fma((float)a, 2^-32, 2^-33): the u32 -> f32 conversion rounds to nearest even (exact below 2^24), so
//                   u in [2^-33, 1] with full resolution where the tail is; u == 1 gives the radius 0, never a NaN
//   angle, in turns (b >> 8) 2^-24, exact; its 32nd parts are split in integers: k = rint(32 turns) picks the row of sct and
//                   32 turns - k = (fi - 2^26) 2^-27 with fi = (b + 2^26) & 0x07FFFF00 is exact in binary32
//   z0 = fma(R, cos, +0), z1 = fma(R, sin, +0) with R = sqrt(-2 log u): |z| <= sqrt(66 ln 2) = 6.7637 (u = 2^-33).  (The fma
//                   against +0: a plain product could be contracted with the caller's next addition, and the draw a simulator
//                   sees would no longer be a rounded value a CPU can restate; a -0 becomes +0.)
// Every step is an exact bit operation, a read of the f64 tables in LDS (RngTables, unchanged) rounded to binary32, an fma / mul /
// add in binary32, or the correctly rounded square root: tests/elementary_f32_ref.py restates it in NumPy and the device gives
// those bits (tests/test_gpu_f32_draws.py).  No v_log_f32 / v_sin_f32 / v_cos_f32 / v_rcp_f32 / v_rsq_f32.
// The two pairs of a block run side by side in the halves of packed instructions (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32):
// left to itself the compiler packs next to nothing here, so the values are spelled as two-element vectors.
// Worst error of a normal against exact arithmetic applied to the same u and angle, measured by tests/test_f32_draws.py over
// its edge words and 2e5 random ones: 3.53 ulp of binary32 (asserted: 4).
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

namespace f32 {

__device__ __forceinline__ f32x2 fma2(const f32x2 a, const f32x2 b, const f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 splat(const float v) { return f32x2{v, v}; }
__device__ __forceinline__ f32x2 as_f32(const u32x2 v) { return f32x2{__uint_as_float(v.x), __uint_as_float(v.y)}; }
__device__ __forceinline__ u32x2 as_u32(const f32x2 v) { return u32x2{__float_as_uint(v.x), __float_as_uint(v.y)}; }

// the correctly rounded sqrt(x) for x = 0 or a normal x (here: x in [6e-8, 46]): v_sqrt_f32 is within one ulp, so the root is the
// seed or one of its neighbours, and the signs of two exact residuals say which -- x - y_down y <= 0: the neighbour below,
// x - y_up y > 0: the one above.  (What the compiler emits for sqrtf(), minus the scaling of tiny inputs.  x = 0: the seed is 0,
// its lower neighbour a NaN whose comparison fails, the upper one's residual is 0: the result is 0.)
__device__ __forceinline__ f32x2 sqrt_cr(const f32x2 x) {
  const f32x2 y = f32x2{__builtin_amdgcn_sqrtf(x.x), __builtin_amdgcn_sqrtf(x.y)};
  const f32x2 yd = as_f32(as_u32(y) - 1u), yu = as_f32(as_u32(y) + 1u);
  const f32x2 rd = fma2(-yd, y, x), ru = fma2(-yu, y, x);
  f32x2 r;
  r.x = rd.x <= 0.0f ? yd.x : y.x;
  r.y = rd.y <= 0.0f ? yd.y : y.y;
  r.x = ru.x > 0.0f ? yu.x : r.x;
  r.y = ru.y > 0.0f ? yu.y : r.y;
  return r;
}

// The rows of RngTables rounded to binary32, one array per column so that the entries of a block's two pairs load into the two
// halves of a packed operand: 1672 bytes of LDS in the kernels that call for_quads_f32, none in the others (RngTables and the
// kernels' prologue stay as they are).  Filled by for_quads_f32 itself, which runs where a workgroup barrier cannot stand
// (behind a kernel's divergent return, inside a simulator): the lanes of the wave that are active at the call write ALL rows,
// the r-th active lane rows r, r + count, ..., and a wave reads only after its own writes -- LDS keeps a wave's accesses in
// order.  Other waves of the workgroup write the same rows with the same values at their own time, which changes nothing a
// reader can see.  The conversions (two per lookup with the f64 rows, 16 VALU instructions per trip of the loop) are paid
// once per call.
// The two columns of a table lie 257 words apart: out of reach of the two-address LDS reads (ds_read2_b32: 255 words,
// ds_read2st64_b32: multiples of 64), into which the compiler would merge the reads of lx[i] and ly[i] -- the words of ONE pair
// would land in a register pair, and moves would have to re-pair them for the packed instructions.
struct TablesF32 {
  float lx[128];                 // logt[i].x
  float sn[33];                  // sct[k].x
  float pad[96];
  float ly[128];                 // logt[i].y, at word 257
  float cs[33];                  // sct[k].y, at word 385 = 128 + 257
};
__device__ __forceinline__ TablesF32 &tables_f32() {
  __shared__ TablesF32 t;
  return t;
}
__device__ __forceinline__ void tables_f32_fill() {
  const RngTables &T = rng_tables();
  TablesF32 &t = tables_f32();
  const uint64_t active = __builtin_amdgcn_ballot_w64(true);
  const int count = __popcll(active);
  const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(active >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)active, 0u));
  for (int i = rank; i < 128; i += count) {
    const double2 e = T.logt[i];
    t.lx[i] = (float)e.x;
    t.ly[i] = (float)e.y;
  }
  for (int i = rank; i < 33; i += count) {
    const double2 e = T.sct[i];
    t.sn[i] = (float)e.x;
    t.cs[i] = (float)e.y;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// -2 log(u) for the two radius uniforms of a block, u in [2^-33, 1].  The scheme of neg2_log_tab on the same table, in binary32:
// the 7 leading mantissa bits, rounded, pick the bin; c = u with the mantissa rounded to those bits (a mask), d = u - c is exact,
// s = d (-2 / c) with the table's -2 inv_i rounded to binary32 and scaled by the power of two in its exponent field, and
// -2 log1p(r) = s + s^2 (1/4 + s/12 + s^2/32) (the next term is below 2^-26 of the result).  (Not fma(u, -2 inv, 2): the rounded
// inv_i no longer matches the table's logarithm, 2^-24 absolutely, which is 2^-15 of a result near u = 1.)
// (TAB32: the rows from TablesF32, filled by the caller, and not converted from RngTables -- the same values.)
template <bool TAB32>
__device__ __forceinline__ f32x2 neg2_log(const f32x2 u) {
  const u32x2 t = as_u32(u) + 0x8000u;                  // half a bin: 1 << 15 of the 23 mantissa bits
  const u32x2 tp = t + (75u << 16);                     // carry when the rounded mantissa is >= 53/128
  const u32x2 nE = 127u - (tp >> 23);                   // -E, 0..33
  const u32x2 i = (t >> 16) & 127u;
  f32x2 ex, ey;
  if constexpr (TAB32) {
    const TablesF32 &T = tables_f32();
    ex = f32x2{T.lx[i.x], T.lx[i.y]};
    ey = f32x2{T.ly[i.x], T.ly[i.y]};
  } else {
    const double2 e0 = rng_tables().logt[i.x], e1 = rng_tables().logt[i.y];
    ex = f32x2{(float)e0.x, (float)e1.x};
    ey = f32x2{(float)e0.y, (float)e1.y};
  }
  const f32x2 c = as_f32(t & 0xFFFF0000u);
  ex = as_f32(as_u32(ex) + (nE << 23));
  const f32x2 s = (u - c) * ex;
  f32x2 p = fma2(s, splat(1.0f / 32.0f), splat(1.0f / 12.0f));
  p = fma2(p, s, splat(0.25f));
  const f32x2 l = fma2(s * s, p, s);
  const f32x2 nEf = f32x2{(float)(int)nE.x, (float)(int)nE.y};
  return fma2(nEf, splat(0x1.62e43p+0f), ey) + l;      // 2 ln 2
}

// the normals of one block
template <bool TAB32 = false>
__device__ __forceinline__ void box_muller_quad(const u32x4 w, float &z0, float &z1, float &z2, float &z3) {
  const f32x2 u = fma2(f32x2{(float)w.x, (float)w.z}, splat(0x1p-32f), splat(0x1p-33f));
  const f32x2 R = sqrt_cr(neg2_log<TAB32>(u));
  const u32x2 t2 = u32x2{w.y, w.w} + 0x04000000u;       // + half a 32nd of a turn; wraps to row 0 where row 32 would be
  const u32x2 fi = t2 & 0x07FFFF00u;
  const u32x2 k = t2 >> 27;
  f32x2 S, C;
  if constexpr (TAB32) {
    const TablesF32 &T = tables_f32();
    S = f32x2{T.sn[k.x], T.sn[k.y]};
    C = f32x2{T.cs[k.x], T.cs[k.y]};
  } else {
    const double2 sc0 = rng_tables().sct[k.x], sc1 = rng_tables().sct[k.y];
    S = f32x2{(float)sc0.x, (float)sc1.x};
    C = f32x2{(float)sc0.y, (float)sc1.y};
  }
  // r = (pi / 16) (32 turns - k): one rounding, of the product of the exact difference with the constant
  const f32x2 r = fma2(f32x2{(float)fi.x, (float)fi.y}, splat(0x1.921fb6p-30f), splat(-0x1.921fb6p-4f));
  const f32x2 r2 = r * r;
  const f32x2 sr = fma2(r * r2, fma2(r2, splat(1.0f / 120.0f), splat(-1.0f / 6.0f)), r);     // sin r, |r| <= pi / 32
  const f32x2 q = fma2(r2, splat(1.0f / 24.0f), splat(-0.5f)) * r2;                          // cos r - 1
  const f32x2 sn = fma2(C, sr, fma2(S, q, S));
  const f32x2 cs = fma2(-S, sr, fma2(C, q, C));
  const f32x2 a = fma2(R, cs, splat(0.0f)), b = fma2(R, sn, splat(0.0f));
  z0 = a.x; z1 = b.x; z2 = a.y; z3 = b.y;
}

// four U(0,1) draws of one block: ((w_i >> 9) + 1/2) 2^-23, exact in binary32 and in (0, 1).  (Not 24 bits: (n + 1/2) 2^-24 is
// no binary32 number from n = 2^23 on, and rounded to nearest even the last word, n = 2^24 - 1, gives 1.)
__device__ __forceinline__ void uniform_quad(const u32x4 w, float &u0, float &u1, float &u2, float &u3) {
  const f32x2 a = fma2(f32x2{(float)(w.x >> 9), (float)(w.y >> 9)}, splat(0x1p-23f), splat(0x1p-24f));
  const f32x2 b = fma2(f32x2{(float)(w.z >> 9), (float)(w.w >> 9)}, splat(0x1p-23f), splat(0x1p-24f));
  u0 = a.x; u1 = a.y; u2 = b.x; u3 = b.y;
}

}  // namespace f32

// team_pick_ct for a binary32 value: one DPP move
template <int W, int J>
__device__ __forceinline__ float team_pick_ct_f32(const float v) {
  static_assert((W == 4 || W == 16) && J >= 0 && J < W, "a quad or a row of 16 lanes");
  constexpr int ctrl = W == 4 ? J * 0x55 : 0x150 + J;
  int r = __builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xF, 0xF, true);
  // the move stays a move: folded into a consumer that is a 64-bit instruction (a simulator's (double)z is v_cvt_f64_f32), the
  // quad_perm control is one such instructions do not have, and the compiler's own check then rejects what its combiner made
  asm("" : "+v"(r));
  return __int_as_float(r);
}

// What the element type of a draw decides, for the code a team shares (NormalStream's team loops and fetch, below): how many
// draws a Philox block gives, how its words become normals or uniforms, and the DPP move of one value.
template <class T> struct TeamDraws;
template <> struct TeamDraws<double> {
  static constexpr int kPerBlock = 2;
  static __device__ __forceinline__ void normals(const u32x4 w, double (&g)[2]) { box_muller(w, g[0], g[1]); }
  static __device__ __forceinline__ void uniforms(const u32x4 w, double (&g)[2]) { g[0] = u52(w.x, w.y); g[1] = u52(w.z, w.w); }
  template <int W, int J> static __device__ __forceinline__ double pick_ct(const double v) { return team_pick_ct<W, J>(v); }
};
template <> struct TeamDraws<float> {
  static constexpr int kPerBlock = 4;
  static __device__ __forceinline__ void normals(const u32x4 w, float (&g)[4]) { f32::box_muller_quad(w, g[0], g[1], g[2], g[3]); }
  static __device__ __forceinline__ void uniforms(const u32x4 w, float (&g)[4]) { f32::uniform_quad(w, g[0], g[1], g[2], g[3]); }
  template <int W, int J> static __device__ __forceinline__ float pick_ct(const float v) { return team_pick_ct_f32<W, J>(v); }
};
// the value lane (team base + j) holds, the lane chosen at run time (uniform over the team): a branch per bit of j
template <int W, int J0 = 0, int N = W, class T>
__device__ __forceinline__ T team_pick(const T v, const uint32_t j) {
  if constexpr (N == 1) {
    return TeamDraws<T>::template pick_ct<W, J0>(v);
  } else {
    return (j & (uint32_t)(N / 2)) ? team_pick<W, J0 + N / 2, N / 2>(v, j) : team_pick<W, J0, N / 2>(v, j);
  }
}
// coop: the group of W blocks this lane holds one block of, for the single calls (NormalStream::fetch)
template <class T> struct TeamBuf {
  int block;                     // first block of the group (-1: none) ...
  bool uniform;                  // ... held as uniforms or as normals
  T v[TeamDraws<T>::kPerBlock];
};

// simulated pairs per loop trip of NormalStream::for_pairs with a lane per particle: independent Philox / Box-Muller chains for
// the scheduler (k_update<1,1,1,0>: 92 -> 62 VGPRs, 246 -> ~240 us at n = 1e6); the draws are still handed out in stream order
constexpr int kSimUnroll = 2;

// NormalStream's coop for a lane per particle whose for_pairs stays the plain loop over pair(): the re-spelled loop holds three
// more vector and two more scalar registers; kernels that sit on their register cap (kernels.hpp: update_loop_coop) keep this one
constexpr int kCoopPlainLoop = -1;

template <int... J> struct lane_seq {};
template <int N, int... J> struct make_lane_seq : make_lane_seq<N - 1, N - 1, J...> {};
template <int... J> struct make_lane_seq<0, J...> { using type = lane_seq<J...>; };

// ---- count draws: the algorithms, written once over `next(u, v)`, the source of trial j's block -- the uniforms of the stream's
// next block for NormalStream::poisson / binomial (below), those of block base + 64 i + j for CountDraws.  Every loop has a
// compile-time bound (1000 inversion steps, kCountBlocks trials), so no draw can spin whatever its arguments are.
// (Both take exp and log from this header -- exp_tab 1.79 ulp, log_fast 0.73 ulp, a few dozen instructions each.)
constexpr int kCountBlocks = 64;             // the trial bound of PTRS and BTRS: the blocks a keyed draw owns
constexpr int kMaxCountDraws = 1 << 20;      // the indices one reserve_counts may reserve
constexpr double kMaxCount = 0x1p30;         // the largest lambda | n_trials

namespace count {

// Poisson(lambda), 0 < lambda <= 2^30.  lambda < 10: sequential-search inversion of u0 of ONE block (at most 1000 steps).
// Otherwise Hoermann's PTRS (transformed rejection with squeeze, Insurance: Mathematics and Economics 12, 1993), one block per
// trial, at most 64 trials (then floor(lambda); 1.15 - 1.33 trials per draw).
template <class Next>
__device__ __forceinline__ int poisson_from(const double lambda, Next &&next) {
  double u, v;
  if (lambda < 10.0) {
    next(u, v);
    double p = exp_tab(-lambda), c = p;
    int k = 0;
    while (u >= c && k < 1000) {
      ++k;
      p *= lambda / (double)k;
      c += p;
    }
    return k;
  }
  const double b = 0.931 + 2.53 * sqrt(lambda), a = -0.059 + 0.02483 * b;
  const double inv_alpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
  const double log_lambda = log_fast(lambda), log_inv_alpha = log_fast(inv_alpha);
  for (int trial = 0; trial < kCountBlocks; ++trial) {
    next(u, v);
    const double U = u - 0.5, us = 0.5 - fabs(U);
    const double kf = floor((2.0 * a / us + b) * U + lambda + 0.43);
    if (us >= 0.07 && v <= vr) return (int)kf;
    if (kf < 0.0 || (us < 0.013 && v > us)) continue;
    if (log_fast(v) + log_inv_alpha - log_fast(a / (us * us) + b) <= -lambda + kf * log_lambda - log_factorial(kf)) return (int)kf;
  }
  return (int)floor(lambda);
}

// Binomial(n, p), n >= 1, 0 < p <= 1/2.  n p < 10: sequential-search inversion of u0 of ONE block.  Otherwise Hoermann's BTRS
// (J. Statist. Comput. Simul. 46, 1993), one block per trial, at most 64 trials (then the mode).
template <class Next>
__device__ __forceinline__ int binomial_lower_from(const int n, const double p, Next &&next) {
  const double q = 1.0 - p, r = p / q, nd = (double)n;
  double u, v;
  if (nd * p < 10.0) {
    next(u, v);
    double pk = exp_tab(nd * log_fast(q)), c = pk;                   // (1 - p)^n, n p < 10
    int k = 0;
    while (u >= c && k < n && k < 1000) {                            // (n p < 10: P(k > 1000) = 0 in binary64; the bound is for a u above the rounded sum)
      ++k;
      pk *= r * (double)(n - k + 1) / (double)k;
      c += pk;
    }
    return k;
  }
  const double spq = sqrt(nd * p * q), b = 1.15 + 2.53 * spq, a = -0.0873 + 0.0248 * b + 0.01 * p, c = nd * p + 0.5;
  const double vr = 0.92 - 4.2 / b, alpha = (2.83 + 5.1 / b) * spq, m = floor((nd + 1.0) * p);
  const double log_r = log_fast(r);
  for (int trial = 0; trial < kCountBlocks; ++trial) {
    next(u, v);
    const double U = u - 0.5, us = 0.5 - fabs(U);
    const double kf = floor((2.0 * a / us + b) * U + c);
    if (us >= 0.07 && v <= vr) return (int)kf;
    if (kf < 0.0 || kf > nd) continue;
    // log f(k) / f(m) = log m! + log (n - m)! - log k! - log (n - k)! + (k - m) log r, summed in that order (most trials end at
    // the squeeze above)
    const double lf = log_factorial(m) + log_factorial(nd - m) - log_factorial(kf) - log_factorial(nd - kf);
    if (log_fast(v * alpha / (a / (us * us) + b)) <= lf + (kf - m) * log_r) return (int)kf;
  }
  return (int)m;
}

}  // namespace count

// Count draws KEYED BY AN INDEX (NormalStream::reserve_counts(n), below): draw index i owns the kCountBlocks = 64 blocks
// base + 64 i .. base + 64 i + 63 of the stream's counter, trial j of a draw uses block base + 64 i + j (the inversion: trial 0),
// and the uniforms of a block are those uniform_pair() returns for it.  The generator is counter-based, so a block nobody asks
// for is never computed: the reserved range costs counter space alone.  A draw is therefore a PURE function of (i, its
// parameters) -- cd.poisson(i, lambda) is what rng.poisson(lambda) returns from a lane-per-particle stream positioned at block
// base + 64 i, the same algorithm constant for constant (count::poisson_from above) --, whichever lane computes it, in whatever
// order, with whatever team width, and whether or not the result is kept.  The CALLING LANE computes the blocks with the plain
// stream_block whatever the stream's coop is: no fetch, no DPP, no LDS beyond the elementary functions' tables.  So the lanes of
// a team may draw for different indices side by side (Series::map, fill, zip: a lane draws for the slots it holds), and a draw
// is legal inside Series::recur's f, which stays pure.
// TOTAL: the relay of recur evaluates f on lanes that discard the result, so every argument has a value.  lambda NaN or <= 0: 0;
// lambda > 2^30 is taken as 2^30.  n_trials (any arithmetic type, taken as a double) is clamped to [0, 2^30], a NaN to 0.  p NaN or <= 0: 0; p >= 1:
// the clamped n_trials.  None of those degenerate cases computes a block.  Every loop keeps its bound: 1000 steps, 64 trials.
// i is not checked: an index outside [0, n) reads blocks that belong to other draws of the stream.
struct CountDraws {
  uint64_t seed, pid, iter;
  uint32_t purpose, base;

  // trial j of index i: the uniforms of block base + 64 i + j
  struct Trials {
    const CountDraws &c;
    uint32_t at;
    __device__ __forceinline__ void operator()(double &u, double &v) {
      const u32x4 w = stream_block(c.seed, c.pid, c.purpose, c.iter, at++);
      u = u52(w.x, w.y);
      v = u52(w.z, w.w);
    }
  };
  __device__ __forceinline__ Trials trials(const int i) const { return Trials{*this, base + (uint32_t)kCountBlocks * (uint32_t)i}; }

  __device__ __forceinline__ int poisson(const int i, const double lambda) const {
    if (!(lambda > 0.0)) return 0;
    return count::poisson_from(fmin(lambda, kMaxCount), trials(i));
  }
  // n_trials: any arithmetic type, taken as a double
  template <class T>
  __device__ __forceinline__ int binomial(const int i, const T n_trials, const double p) const {
    const int n = (int)fmin(fmax((double)n_trials, 0.0), kMaxCount);   // (fmax(NaN, 0) = 0)
    if (n <= 0 || !(p > 0.0)) return 0;
    if (p >= 1.0) return n;
    if (p > 0.5) return n - count::binomial_lower_from(n, 1.0 - p, trials(i));
    return count::binomial_lower_from(n, p, trials(i));
  }
};

// Sequential N(0,1) stream of one (particle, purpose, iteration): block k yields normals 2k, 2k+1.
//
// coop = 4 | 16 (k_update_persistent on small shards, persistent_kernel.hpp): the lanes of a TEAM -- a quad, or a row of 16 --
// run the same particle -- the same code on the same data -- and share the generator: each lane turns ITS blocks into pairs
// (the 99 of a simulator's ~105 instructions per pair that are Philox + Box-Muller), and the team consumes the pairs in stream
// order through DPP broadcasts.  The stream a simulator sees is the same stream, pair for pair and bit for bit (counter-based:
// block k is block k whoever computes it); a particle's chain of draws is a quarter | a sixteenth as long.  (Worth it only
// while the device is under-filled: the team issues more instructions per particle than one lane.)  All lanes of a team must
// make the same requests -- they do: their control flow depends on the particle's data only.
//
// for_pairs(n, f) -- f(z0, z1) for the next n pairs of the stream, in stream order -- is the loop a simulator should draw its
// bulk with.  A lane per particle: the loop over the stream's blocks, two trips unrolled, in its
// re-spelled form (namespace loop above; kCoopPlainLoop: the plain loop over pair()).  A team per particle: 4 W pairs at a time,
// FOUR blocks per lane side by side (a single block per lane is a chain of ~100 dependent instructions: with one wave on the
// SIMD its latency, not its issue, is what the team would wait for), handed out through DPP broadcasts whose lane is a
// compile-time constant; the rest -- fewer than 4 W pairs -- in one more group of as many blocks per lane as it takes.  pair() / uniform_pair() / next() keep working in either mode, one
// group of W at a time, the lane picked by branches on the stream position.
//
// The binary32 draws (quad_f32 / uniform_quad_f32 / for_quads_f32) share a stream the same way, a block being four floats where
// it was two doubles: the team loop (for_team, tail, hand_out), fetch and its buffer are written once over the element type, and
// TeamDraws<T> above holds what the type decides.
struct NormalStream {
  uint64_t seed, pid, iter;
  uint32_t purpose, k;
  double spare;
  bool have;
  int coop;                      // 0: every lane its own stream | 4, 16: the lanes of a team share one (see above)
                                 // | kCoopPlainLoop: as 0, with for_pairs as the plain loop over pair()
  TeamBuf<double> buf64;         // coop: the group behind pair / uniform_pair ...
  TeamBuf<float> buf32;          // ... and the one behind quad_f32 / uniform_quad_f32, a buffer of their own
  // where sabc::emit puts the outputs of THIS simulation: output i at out[i * out_stride], i < out_n.  Null from every
  // constructor: only the forward run (Sim<SABC_MODEL_USER>::run_out) sets a destination, so in every other kernel
  // the null is a constant after inlining and what a simulator does for its outputs is dead code there
  double *out;
  long long out_stride, out_n;
  __device__ __forceinline__ NormalStream(uint64_t seed_, uint64_t pid_, uint32_t purpose_, uint64_t iter_, int coop_ = 0)
      : seed(seed_), pid(pid_), iter(iter_), purpose(purpose_), k(0), spare(0.0), have(false), coop(coop_),
        buf64{-1, false, {}}, buf32{-1, false, {}}, out(nullptr), out_stride(0), out_n(0) {}
  __device__ __forceinline__ void set_outputs(double *out_, long long stride_, long long n_) {
    out = out_;
    out_stride = stride_;
    out_n = out_ ? n_ : 0;
  }
  __device__ __forceinline__ void pair(double &z0, double &z1) {  // consumes one whole block
    double g[2];
    if (coop == 4) fetch<4>(k++, false, buf64, g);
    else if (coop == 16) fetch<16>(k++, false, buf64, g);
    else TeamDraws<double>::normals(stream_block(seed, pid, purpose, iter, k++), g);
    z0 = g[0]; z1 = g[1];
  }
  // two U(0,1) draws from one whole block (the 52-bit uniforms the Box-Muller pair would have been made of)
  __device__ __forceinline__ void uniform_pair(double &u0, double &u1) {
    double g[2];
    if (coop == 4) fetch<4>(k++, true, buf64, g);
    else if (coop == 16) fetch<16>(k++, true, buf64, g);
    else TeamDraws<double>::uniforms(stream_block(seed, pid, purpose, iter, k++), g);
    u0 = g[0]; u1 = g[1];
  }
  template <class F>
  __device__ __forceinline__ void for_pairs(const int n, F &&f) {
    if (coop == 0) { for_pairs_lane(n, f); return; }
    for_pairs_plain(n, f);
  }
  // ---- binary32 draws (namespace f32 above): each call consumes WHOLE blocks of the same stream and the same counter k, so they
  // mix freely with pair(), uniform_pair(), while_events and the count draws.  |z| <= 6.7637.
  // four N(0,1) from one block: (z0, z1) from its words (x, y), (z2, z3) from (z, w)
  __device__ __forceinline__ void quad_f32(float &z0, float &z1, float &z2, float &z3) {
    float g[4];
    if (coop == 4) fetch<4>(k++, false, buf32, g);
    else if (coop == 16) fetch<16>(k++, false, buf32, g);
    else TeamDraws<float>::normals(stream_block(seed, pid, purpose, iter, k++), g);
    z0 = g[0]; z1 = g[1]; z2 = g[2]; z3 = g[3];
  }
  // four U(0,1) from one block: u_i = ((w_i >> 9) + 1/2) 2^-23, exact, in (0, 1)
  __device__ __forceinline__ void uniform_quad_f32(float &u0, float &u1, float &u2, float &u3) {
    float g[4];
    if (coop == 4) fetch<4>(k++, true, buf32, g);
    else if (coop == 16) fetch<16>(k++, true, buf32, g);
    else TeamDraws<float>::uniforms(stream_block(seed, pid, purpose, iter, k++), g);
    u0 = g[0]; u1 = g[1]; u2 = g[2]; u3 = g[3];
  }
  // f(z0, z1, z2, z3) for the next n blocks of the stream, in stream order: the loop to draw the bulk of binary32 normals with
  template <class F>
  __device__ __forceinline__ void for_quads_f32(const int n, F &&f) {
    if (coop == 4) { for_team<float, 4>(n, f); return; }
    if (coop == 16) { for_team<float, 16>(n, f); return; }
    if (coop == 0) {                                     // a lane per particle: the re-spelled block generator (namespace loop)
      f32::tables_f32_fill();                            // ... and the tables in binary32, converted once per call
#pragma unroll kSimUnroll
      for (int i = 0; i < n; ++i) {
        float z0, z1, z2, z3;
        f32::box_muller_quad<true>(loop::stream_block(seed, pid, purpose, iter, k++), z0, z1, z2, z3);
        f(z0, z1, z2, z3);
      }
      return;
    }
#pragma unroll kSimUnroll
    for (int i = 0; i < n; ++i) {                        // kCoopPlainLoop
      float z0, z1, z2, z3;
      quad_f32(z0, z1, z2, z3);
      f(z0, z1, z2, z3);
    }
  }
  __device__ __forceinline__ double next() {
    if (have) { have = false; return spare; }
    double z0;
    pair(z0, spare);
    have = true;
    return z0;
  }

  // ---- draws for discrete-event and count models (Gillespie, tau-leaping, chain-binomial).  Each consumes WHOLE blocks of the
  // stream, like pair(): (u0, u1) below are the uniforms uniform_pair() would have returned for the same block. ----

  // two Exp(1) draws from one block: e_i = -log(u_i), the log from the LDS table (neg2_log_tab, 1.87 ulp at the worst)
  __device__ __forceinline__ void exponential_pair(double &e0, double &e1) {
    double u0, u1;
    uniform_pair(u0, u1);
    e0 = 0.5 * neg2_log_tab(u0);
    e1 = 0.5 * neg2_log_tab(u1);
  }
  // one step of Gillespie's direct method from one block: the waiting time e = -log(u0) (to be divided by the total rate) and
  // the uniform u = u1 that picks the event
  __device__ __forceinline__ void event_pair(double &e, double &u) {
    double u0;
    uniform_pair(u0, u);
    e = 0.5 * neg2_log_tab(u0);
  }
  // f(e, u) -> bool with the event pairs of successive blocks, in stream order, until f returns false or max_events calls are
  // made; returns the number of calls, and the stream has advanced by exactly that many blocks.  The loop a simulator whose trip
  // count depends on its draws should use: a lane per particle runs the re-spelled block generator with its constants loaded
  // once; a team of 4 | 16 lanes turns a group of W blocks into (e, u) side by side, one block per lane, log included, and
  // consumes them through DPP broadcasts with compile-time lanes, dropping the rest of the group at the first false (all
  // lanes of a team see the same data, so the exit is uniform over the team).
  template <class F>
  __device__ __forceinline__ int while_events(const int max_events, F &&f) {
    if (coop == 4) return while_events_team<4>(max_events, f);
    if (coop == 16) return while_events_team<16>(max_events, f);
    if (coop == 0) return while_events_lane(max_events, f);
    int count = 0;
    while (count < max_events) {
      double e, u;
      event_pair(e, u);
      ++count;
      if (!f(e, u)) break;
    }
    return count;
  }
  // Poisson(lambda), lambda <= 2^30.  lambda <= 0: 0, no block.  lambda < 10: inversion of u0 of ONE block; otherwise PTRS, one
  // block per trial, at most 64 (count::poisson_from above, on the stream's next blocks).
  __device__ __forceinline__ int poisson(const double lambda) {
    if (!(lambda > 0.0)) return 0;
    return count::poisson_from(lambda, [&](double &u, double &v) { uniform_pair(u, v); });
  }
  // Binomial(n, p).  n <= 0 or p <= 0: 0, p >= 1: n, no block.  p > 1/2: n - binomial(n, 1 - p).  n p < 10: inversion of u0 of
  // ONE block; otherwise BTRS, one block per trial, at most 64 (count::binomial_lower_from above, on the stream's next blocks).
  __device__ __forceinline__ int binomial(const int n, const double p) {
    if (n <= 0 || !(p > 0.0)) return 0;
    if (p >= 1.0) return n;
    const auto next = [&](double &u, double &v) { uniform_pair(u, v); };
    if (p > 0.5) return n - count::binomial_lower_from(n, 1.0 - p, next);
    return count::binomial_lower_from(n, p, next);
  }
  // n draw indices 0 .. n - 1 for count draws keyed by an index (CountDraws above): records (seed, pid, purpose, iter, base = k)
  // and advances k by kCountBlocks n = 64 n.  No block is generated.  0 <= n <= 2^20 = kMaxCountDraws: checked at compile time in
  // the template form, clamped in the other.  THE COUNTER BUDGET: k has 32 bits, 2^32 blocks per (particle, purpose, iteration);
  // a reservation of 2^20 indices takes 2^26 of them, and nothing checks the sum of a simulator's requests.
  // The team buffers (buf64, buf32) and next()'s spare stay as they are: fetch compares the group of the block it is asked for
  // with the group it holds and refills by itself when k has left it, and the spare is the second normal of a block consumed
  // before the reservation, still the stream's next normal for next().
  __device__ __forceinline__ CountDraws reserve_counts(const int n) {
    const CountDraws cd{seed, pid, iter, purpose, k};
    k += (uint32_t)kCountBlocks * (uint32_t)(n < 0 ? 0 : n > kMaxCountDraws ? kMaxCountDraws : n);
    return cd;
  }
  template <int N>
  __device__ __forceinline__ CountDraws reserve_counts() {
    static_assert(N >= 0 && N <= kMaxCountDraws, "reserve_counts: 0 <= n <= 2^20 draw indices");
    return reserve_counts(N);
  }

 private:
  // a lane per particle: the loop over the stream's blocks in its re-spelled form (namespace loop; same bits as event_pair)
  template <class F>
  __device__ __forceinline__ int while_events_lane(const int max_events, F &f) {
    const loop::Regs c = loop::Regs::load();
    int count = 0;
    while (count < max_events) {
      const u32x4 w = loop::stream_block(seed, pid, purpose, iter, k++);
      const double e = 0.5 * loop::neg2_log_tab(loop::u52(w.x, w.y, c));
      ++count;
      if (!f(e, loop::u52(w.z, w.w, c))) break;
    }
    return count;
  }
  // a lane per particle, the re-spelled loop (namespace loop)
  template <class F>
  __device__ __forceinline__ void for_pairs_lane(const int n, F &f) {
    const loop::Regs c = loop::Regs::load();           // once per loop, not per pair
#pragma unroll kSimUnroll
    for (int i = 0; i < n; ++i) {
      double z0, z1;
      loop::box_muller(loop::stream_block(seed, pid, purpose, iter, k++), z0, z1, c);
      f(z0, z1);
    }
  }
  // a team per particle, or a lane per particle with the plain loop over pair() (kCoopPlainLoop)
  template <class F>
  __device__ __forceinline__ void for_pairs_plain(const int n, F &&f) {
    if (coop == 4) { for_team<double, 4>(n, f); return; }
    if (coop == 16) { for_team<double, 16>(n, f); return; }
#pragma unroll kSimUnroll
    for (int i = 0; i < n; ++i) {
      double z0, z1;
      pair(z0, z1);
      f(z0, z1);
    }
  }
  // ---- a team per particle
  // the events of one group, lane J's after lane J - 1's, while f says go on and the bound allows
  template <int W, class F, int... J>
  __device__ __forceinline__ bool hand_out_events(const double ge, const double gu, const int max_events, int &count, F &f, lane_seq<J...>) {
    bool go = true;
    ((go = go && count < max_events && (++count, f(team_pick_ct<W, J>(ge), team_pick_ct<W, J>(gu)))), ...);
    return go;
  }
  // blocks k + count + q on lane q, one block per lane per group
  template <int W, class F>
  __device__ __forceinline__ int while_events_team(const int max_events, F &f) {
    using lanes = typename make_lane_seq<W>::type;
    const uint32_t q = threadIdx.x & (uint32_t)(W - 1);
    int count = 0;
    bool go = true;
    while (go && count < max_events) {
      const u32x4 w = stream_block(seed, pid, purpose, iter, k + (uint32_t)count + q);
      const double ge = 0.5 * neg2_log_tab(u52(w.x, w.y)), gu = u52(w.z, w.w);
      go = hand_out_events<W>(ge, gu, max_events, count, f, lanes{});
    }
    k += (uint32_t)count;
    return count;
  }
  // for_pairs and for_quads_f32 (T = double | float): f with the normals of one block per lane, lane J's after lane J - 1's,
  // for the first m <= W lanes (m = W, a constant where it is called: all of them, no comparison left).
  // (The arity of f is spelled in place: through a helper per lane, one call deeper, the binary32 tail compiles differently.)
  template <class T, int W, class F, int... J>
  __device__ __forceinline__ void hand_out(const int m, const T (&g)[TeamDraws<T>::kPerBlock], F &f, lane_seq<J...>) {
    using D = TeamDraws<T>;
    if constexpr (D::kPerBlock == 2) ((J < m ? f(D::template pick_ct<W, J>(g[0]), D::template pick_ct<W, J>(g[1])) : (void)0), ...);
    else ((J < m ? f(D::template pick_ct<W, J>(g[0]), D::template pick_ct<W, J>(g[1]), D::template pick_ct<W, J>(g[2]), D::template pick_ct<W, J>(g[3])) : (void)0), ...);
  }
  template <class T, int W, int NB, class F>
  __device__ __forceinline__ void tail(const int c, const int r, F &f) {      // (NB - 1) W < r <= NB W blocks from block k + c on
    using lanes = typename make_lane_seq<W>::type;
    const uint32_t q = threadIdx.x & (uint32_t)(W - 1);
    T g[NB][TeamDraws<T>::kPerBlock];
#pragma unroll
    for (int a = 0; a < NB; ++a) TeamDraws<T>::normals(stream_block(seed, pid, purpose, iter, k + (uint32_t)(c + W * a) + q), g[a]);
#pragma unroll
    for (int a = 0; a < NB - 1; ++a) hand_out<T, W>(W, g[a], f, lanes{});
    hand_out<T, W>(r - (NB - 1) * W, g[NB - 1], f, lanes{});
  }
  template <class T, int W, class F>
  __device__ __forceinline__ void for_team(const int n, F &f) {
    using lanes = typename make_lane_seq<W>::type;
    const uint32_t q = threadIdx.x & (uint32_t)(W - 1);
    int c = 0;
    for (; c + 4 * W <= n; c += 4 * W) {               // whole groups of 4 W: blocks k + c + W a + q, a = 0..3, on lane q
      T g[4][TeamDraws<T>::kPerBlock];
#pragma unroll
      for (int a = 0; a < 4; ++a) TeamDraws<T>::normals(stream_block(seed, pid, purpose, iter, k + (uint32_t)(c + W * a) + q), g[a]);
#pragma unroll
      for (int a = 0; a < 4; ++a) hand_out<T, W>(W, g[a], f, lanes{});
    }                                                  // (not tail<T, W, 4>(c, 4 W, f): the team kernels compile differently)
    const int r = n - c;                               // the rest, < 4 W blocks: ceil(r / W) blocks per lane, again side by side
    if (r > 3 * W) tail<T, W, 4>(c, r, f);
    else if (r > 2 * W) tail<T, W, 3>(c, r, f);
    else if (r > W) tail<T, W, 2>(c, r, f);
    else if (r > 0) tail<T, W, 1>(c, r, f);
    k += (uint32_t)n;
  }
  // coop: block kk of the stream, from the lane of the team that holds it; a group of W blocks is (re)generated -- one block
  // per lane -- when the request leaves the buffered group or asks for the other kind (a simulator that mixes pair() and
  // uniform_pair() inside a group pays a refill for it, the stream it sees is still the stream)
  template <int W, class T>
  __device__ __forceinline__ void fetch(uint32_t kk, bool uniform, TeamBuf<T> &b, T (&x)[TeamDraws<T>::kPerBlock]) {
    const int base = (int)(kk & ~(uint32_t)(W - 1));
    if (b.block != base || b.uniform != uniform) {
      const u32x4 w = stream_block(seed, pid, purpose, iter, (uint32_t)base + (threadIdx.x & (uint32_t)(W - 1)));
      if (uniform) TeamDraws<T>::uniforms(w, b.v);
      else TeamDraws<T>::normals(w, b.v);
      b.block = base;
      b.uniform = uniform;
    }
#pragma unroll
    for (int i = 0; i < TeamDraws<T>::kPerBlock; ++i) x[i] = team_pick<W>(b.v[i], kk);
  }
};

// ---- outputs of a simulator from source (sabc_op_simulate_outputs).  The stream is the one per-simulation object a
// simulator has, so it carries the destination.  emitting: false in every kernel but a forward run that asked for outputs --
// the guard for bookkeeping that exists for the outputs only.  emit: output i of THIS simulation; nothing when not emitting,
// and nothing for an i outside [0, n_outputs): the index IS checked (unlike data_at's), a stray store would land in another
// simulation's outputs or behind the buffer.  What is never emitted reads as NaN on the host.
__device__ __forceinline__ bool emitting(const NormalStream &rng) { return rng.out != nullptr; }
__device__ __forceinline__ long long n_outputs(const NormalStream &rng) { return rng.out ? rng.out_n : 0; }
__device__ __forceinline__ void emit(NormalStream &rng, const long long i, const double v) {
  if (rng.out && i >= 0 && i < rng.out_n) rng.out[i * rng.out_stride] = v;
}

}  // namespace sabc

#include "team_sample.hpp"     // sabc::Sample<N, W>: a sample spread over the lanes of a team (uses NormalStream, team_pick and emit above)
#include "team_sample_f32.hpp" // sabc::SampleF32<N, W>: its binary32 twin, four normals per block (f32::box_muller_quad, team_pick)
#include "team_series.hpp"     // sabc::Series<N, W>: a time series in time order over the team, lags through DPP (uses the above)
