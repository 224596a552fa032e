"""What the binary32 draws buy (NormalStream::for_quads_f32, csrc/device_rng.hpp namespace f32) against the f64 ones, on one
box with the two forms alternating inside this process:

  peak      sabc_op_rng_peak against sabc_op_rng_peak_f32, normals/s at the lane count of bench.py's pre-heat (1e6 lanes, 100 normals
            per lane), --regions calls each
  update    us per population update of LotkaVolterraF32 against the same model written as a DeviceSource in f64 (below: the
            step of Sim<SABC_MODEL_LV> through for_pairs): n = 1e6 on the launch chain, n = 1000 in one launch with the engine's
            own choice of lanes and with SABC_PERSISTENT_LANES = 4 and 16; RandomWalk, a warm-up region, then --regions regions
            of --updates updates per form
  code      VGPRs, occupancy and VALU instructions per trip of the two loops, from the code objects hipcc makes of
            tests/generator_isa/*.hip

No threshold: the file records the measured ratio next to the instruction-count ratio.

    python tools/f32_draws_ab.py --out profiles/f32_draws_ab.txt
"""
import argparse
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LV_OBS = (18.0, 17.0, 14.0, 12.0)
LV_HI = (2.0, 0.1, 2.0)

# Sim<SABC_MODEL_LV>::run (csrc/device_models.hpp) as a simulator from source: the f64 side of the comparison
LV_F64_SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const int n_steps = (int)p[0];
  const double dt = p[1], sdt = p[2] * sqrt(p[1]);
  double X = p[3], Y = p[4], SX = 0, QX = 0, SY = 0, QY = 0;
  rng.for_pairs(n_steps, [&](const double z1, const double z2) {
    const double fx = fma(sdt, z1, fma(-theta[1], Y, theta[0]) * dt);
    const double fy = fma(sdt, z2, fma(theta[1], X, -theta[2]) * dt);
    X = fmax(fma(X, fx, X), 0.0);
    Y = fmax(fma(Y, fy, Y), 0.0);
    SX += X; QX += X * X; SY += Y; QY += Y * Y;
  });
  const double mX = SX / n_steps, mY = SY / n_steps;
  const double vX = (QX - SX * mX) / (n_steps - 1), vY = (QY - SY * mY) / (n_steps - 1);
  const double st[4] = {mX, sqrt(fmax(vX, 0.0)), mY, sqrt(fmax(vY, 0.0))};
  for (int j = 0; j < 4; ++j) {
    const double d = fabs(st[j] - p[5 + j]);
    rho[j] = d < 1e300 ? d : 1e300;
  }
}
"""


def loop_figures(say):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        say("code: no hipcc here")
        return None
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_generator_isa import basic_blocks
    csrc = os.path.join(ROOT, "simulatedannealingabc.jl_amd", "csrc")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, kernel, per_trip in (("for_pairs_sum", "k_for_pairs_sum", 4), ("for_quads_f32_sum", "k_for_quads_f32_sum", 8)):
            asm_path = os.path.join(tmp, name + ".s")
            subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", f"-I{csrc}",
                            os.path.join(ROOT, "tests", "generator_isa", name + ".hip"), "-o", asm_path], check=True, capture_output=True)
            asm = open(asm_path, encoding="utf-8").read()
            loop = max(basic_blocks(asm, kernel), key=lambda b: sum(op == "v_mad_u64_u32" for op in b))
            valu = sum(op.startswith("v_") for op in loop)
            tail = asm.split(f"\n{kernel}:", 1)[1]
            fig = {k: int(re.search(rf"; {k}: (\d+)", tail).group(1)) for k in ("NumVgprs", "Occupancy", "ScratchSize", "LDSByteSize")}
            out[name] = valu / per_trip
            say(f"code: {kernel}: {valu} VALU per trip = {valu / per_trip:g} per normal, {sum(op.startswith('v_pk_') for op in loop)} packed; "
                f"VGPRs {fig['NumVgprs']}, occupancy {fig['Occupancy']}, LDS {fig['LDSByteSize']} B, scratch {fig['ScratchSize']}")
    return out["for_pairs_sum"] / out["for_quads_f32_sum"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f32_draws_ab.txt"))
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20241220)
    args = ap.parse_args()
    import sabc_amd as S
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# tools/f32_draws_ab.py: f64 and binary32 forms alternating in one process, {args.regions} regions each")
    count_ratio = loop_figures(say)
    if count_ratio:
        say(f"code: instructions per normal, f64 / f32 = {count_ratio:.3f}")

    # ---- the bare loops
    S.op_rng_peak(1_000_000, 50, 20)
    S.op_rng_peak_f32(1_000_000, 25, 20)
    peak = dict(f64=[], f32=[])
    for _ in range(args.regions):
        peak["f64"].append(S.op_rng_peak(1_000_000, 50, 20))
        peak["f32"].append(S.op_rng_peak_f32(1_000_000, 25, 20))
    med = {k: statistics.median(v) for k, v in peak.items()}
    say(f"peak: 1e6 lanes x 100 normals, 20 launches per call: f64 {med['f64']:.4g} normals/s (regions " + " ".join(f"{x:.4g}" for x in peak["f64"])
        + f") | f32 {med['f32']:.4g} (" + " ".join(f"{x:.4g}" for x in peak["f32"]) + f") | f32 / f64 = {med['f32'] / med['f64']:.3f}")

    # ---- the Lotka-Volterra update
    prior = S.product_distribution([S.Uniform(0.0, hi) for hi in LV_HI])
    params = [256, 0.05, 0.1, 50.0, 50.0, *LV_OBS]
    say("# n  form  us/update f64 (median, spread)  us/update f32 (median, spread)  f64 / f32")
    for n, persistent, lanes in ((1_000_000, "0", None), (1000, "1", None), (1000, "1", 4), (1000, "1", 16)):
        os.environ["SABC_PERSISTENT"] = persistent            # read when the handle is created
        os.environ["SABC_PERSISTENT_MAX"] = "65536"
        if lanes:
            os.environ["SABC_PERSISTENT_LANES"] = str(lanes)
        else:
            os.environ.pop("SABC_PERSISTENT_LANES", None)
        models = dict(f64=S.DeviceSource(LV_F64_SRC, 3, 4, params), f32=S.LotkaVolterraF32(obs=LV_OBS))
        handles = {k: S.SabcHandle(n_particles=n, model=m, prior=prior, seed=args.seed) for k, m in models.items()}
        for h in handles.values():
            h.initialize(n)
            h.update(n_simulation=args.updates * n, proposal=S.RandomWalk(n_para=3))        # warm-up: as long as a timed region
        times = dict(f64=[], f32=[])
        for _ in range(args.regions):
            for k, h in handles.items():
                t0 = time.perf_counter()
                h.update(n_simulation=args.updates * n, proposal=S.RandomWalk(n_para=3))
                times[k].append((time.perf_counter() - t0) / args.updates * 1e6)
        form = "launch chain" if persistent == "0" else f"one launch ({handles['f32'].persistent_lanes} lanes)"
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = {k: max(v) - min(v) for k, v in times.items()}
        say(f"update: n={n:8d} {form:22s} f64 {med['f64']:10.2f} ({spread['f64']:8.2f})  f32 {med['f32']:10.2f} ({spread['f32']:8.2f})  "
            f"f64 / f32 = {med['f64'] / med['f32']:.3f}")
        if persistent == "0":
            say(f"    normals drawn per second: f64 {n * 512 / (med['f64'] * 1e-6):.4g}, f32 {n * 512 / (med['f32'] * 1e-6):.4g}")
        say("    regions f64: " + " ".join(f"{x:.2f}" for x in times["f64"]) + " | f32: " + " ".join(f"{x:.2f}" for x in times["f32"]))
        for h in handles.values():
            h.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
