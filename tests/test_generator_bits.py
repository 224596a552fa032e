"""The generator's outputs, bit for bit, against fixtures recorded with the build BEFORE its hot loop was trimmed.

The trim (device_rng.hpp: the wave-uniform half of Philox rounds 1-2 on the scalar unit, the loop's literals held in
registers, a three-address FMA) re-spells code without changing arithmetic: same products, same FMAs, same order.  Re-spelling
can change what the compiler contracts or reorders, so this is checked, not assumed: tests/golden/generator_bits/*.npy hold
what the parent build computed on an MI355X (manifest.json names the commit), as uint64 views of the float64 results, and
every build since has to reproduce them exactly:

  pairs     op_normal_pairs (the free box_muller): several seeds / purposes / iterations / block indices, large pids included
  simulate  h.simulate() distances of the built-in models at 300 thetas each (NormalStream::for_pairs with its fused sums; the
            g-and-k simulators' own draws)
  chain     a 2000-particle, 40-update cfg2 run through the launch chain and through the one-launch form with 1 / 4 / 16 lanes
            per particle: final theta, u, rho, epsilon and the per-update history

Re-recorded once since, on purpose: neg2_log_tab rounded its mantissa by a quarter of a bin instead of half (tests/
test_elementary_functions.py), and the correction moves about a quarter of all table logs to another table entry.  The pairs
whose first uniform stays in its bin kept both values bit for bit, the others moved by 2 ulp at the most (manifest.json,
"rerecorded").

Recording (on a GPU, with the build to record from):  python tests/test_generator_bits.py --record <commit>"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "generator_bits")
SEED = 20241220          # fixed: the fixtures are recorded with it (tests/cases.py lets SABC_TEST_SEED move its own)

PAIRS = [  # (seed, pid0, m, purpose, iteration, block index)
    (SEED, 0, 1024, 1, 0, 0),
    (SEED, 999_000, 1024, 1, 37, 49),
    (7, 2 ** 33 + 5, 512, 2, 3, 1),
    (2 ** 63 + 12345, 2 ** 40 - 100, 512, 3, 2 ** 32 + 9, 7),
    (1, 123_456_789, 512, 4, 1_000_000, 0),
    (0xDEADBEEFCAFE, 2 ** 32 - 256, 512, 0, 0, 2 ** 31 + 3),
    (42, 17, 512, 5, 11, 255),
]
SIMULATE = ["gauss1_cfg2", "gauss1_2stats", "gauss2_2stats", "gauss2d_cfg3", "gk_cfg4", "gk_c09", "lv_cfg5"]
SIM_BOX = {"N": lambda a, b: (a - 2 * b, a + 2 * b), "U": lambda a, b: (a + 0.02 * (b - a), b - 0.02 * (b - a))}
CHAIN = [("chain", {"SABC_PERSISTENT": "0"}), ("lanes1", {"SABC_PERSISTENT": "1", "SABC_PERSISTENT_LANES": "1"}),
         ("lanes4", {"SABC_PERSISTENT": "1", "SABC_PERSISTENT_LANES": "4"}),
         ("lanes16", {"SABC_PERSISTENT": "1", "SABC_PERSISTENT_LANES": "16"})]
CHAIN_N, CHAIN_UPDATES = 2000, 40


def model_prior(S, name):
    from tests.cases import MODELS
    spec = MODELS[name]
    kind, kw = spec["model"]
    if name == "gauss1_cfg2":          # tests/cases.py derives this one's observation from ITS seed
        kw = dict(kw, obs_mean=float(np.random.default_rng(SEED).normal(1.5, 1.0, 100).mean()))
    comps = [S.Normal(p[1], p[2]) if p[0] == "N" else S.Uniform(p[1], p[2]) for p in spec["prior"]]
    return getattr(S, kind)(**kw), (comps[0] if len(comps) == 1 else S.product_distribution(comps)), spec


def compute_pairs(S):
    return {f"pairs{i}": S.op_normal_pairs(seed, pid0, m, purpose=purpose, it=it, k=k)
            for i, (seed, pid0, m, purpose, it, k) in enumerate(PAIRS)}


def compute_simulate(S):
    out = {}
    for j, name in enumerate(SIMULATE):
        model, prior, spec = model_prior(S, name)
        rng = np.random.default_rng(100 + j)
        lo, hi = np.array([SIM_BOX[p[0]](p[1], p[2]) for p in spec["prior"]]).T
        theta = lo[:, None] + (hi - lo)[:, None] * rng.random((len(lo), 300))
        h = S.SabcHandle(n_particles=256, model=model, prior=prior, seed=SEED)
        out[f"sim_{name}_theta"] = theta
        out[f"sim_{name}"] = h.simulate(theta, pid0=(2 ** 34 + 77) if j % 2 else 5000, it=3 + j)
        h.close()
    return out


def compute_chain(S, tag, env):
    saved = {k: os.environ.get(k) for k in ("SABC_PERSISTENT", "SABC_PERSISTENT_LANES", "SABC_PERSISTENT_MAX")}
    try:
        for k in saved:
            os.environ.pop(k, None)
        os.environ.update(env)
        model, prior, _ = model_prior(S, "gauss1_cfg2")
        h = S.SabcHandle(n_particles=CHAIN_N, model=model, prior=prior, seed=SEED)
        h.initialize(CHAIN_N)
        h.update(n_simulation=CHAIN_UPDATES * CHAIN_N, proposal=S.RandomWalk(n_para=1))
        theta, u, rho = h.get_population()
        eps_h, u_h, rho_h = h.history
        c = h.counters
        lanes = h.persistent_lanes
        out = {"theta": theta, "u": u, "rho": rho, "eps": np.atleast_1d(h.eps), "eps_history": eps_h, "u_history": u_h,
               "rho_history": rho_h,
               "counters": np.array([c["n_simulation"], c["n_accept"], c["n_resampling"], c["n_population_updates"]], dtype=np.float64)}
        h.close()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    want = int(env.get("SABC_PERSISTENT_LANES", 0)) if env["SABC_PERSISTENT"] == "1" else 0
    assert lanes == want, f"{tag}: ran with {lanes} lanes per particle, not {want}"
    assert out["counters"][3] == CHAIN_UPDATES and out["counters"][1] > 0
    return {f"{tag}_{k}": np.asarray(v, dtype=np.float64) for k, v in out.items()}


GROUPS = {"pairs": compute_pairs, "simulate": compute_simulate,
          "chain": lambda S: {k: v for tag, env in CHAIN for k, v in compute_chain(S, tag, env).items()}}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).ravel()


def load(group):
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        manifest = json.load(f)
    flat = np.load(os.path.join(GOLDEN, f"{group}.npy"))
    assert flat.dtype == np.uint64
    return {e["key"]: (flat[e["offset"]: e["offset"] + int(np.prod(e["shape"]))], tuple(e["shape"]))
            for e in manifest["groups"][group]}


def check(group, got):
    want = load(group)
    assert sorted(want) == sorted(got), (sorted(want), sorted(got))
    bad = []
    for key, (w, shape) in want.items():
        g = np.asarray(got[key])
        assert g.shape == shape, (key, g.shape, shape)
        if not np.array_equal(bits(g), w):
            n = int((bits(g) != w).sum())
            rel = np.max(np.abs(g.ravel() - w.view(np.float64)) / np.maximum(np.abs(w.view(np.float64)), 1e-300))
            bad.append(f"{key}: {n} of {w.size} values differ (largest relative difference {rel:.3g})")
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_normal_pairs_reproduce_the_parent_build(S, gpu):
    got = compute_pairs(S)
    assert sum(len(v) for v in got.values()) >= 4000
    check("pairs", got)


@pytest.mark.gpu
def test_simulated_distances_reproduce_the_parent_build(S, gpu):
    check("simulate", compute_simulate(S))


@pytest.mark.gpu
@pytest.mark.parametrize("tag,env", CHAIN, ids=[t for t, _ in CHAIN])
def test_cfg2_chain_reproduces_the_parent_build(S, gpu, tag, env):
    want = {k: v for k, v in load("chain").items() if k.startswith(tag + "_")}
    got = compute_chain(S, tag, env)
    assert sorted(want) == sorted(got)
    bad = [k for k, (w, shape) in want.items() if got[k].shape != shape or not np.array_equal(bits(got[k]), w)]
    assert not bad, f"differ from the parent build's: {bad}"


def record(commit):
    import sabc_amd as S
    S.build()
    os.makedirs(GOLDEN, exist_ok=True)
    manifest = {"recorded_with": commit, "device": "AMD Instinct MI355X (gfx950)",
                "note": "float64 results of the build named in recorded_with, as uint64 views, concatenated per group; "
                        "written by `python tests/test_generator_bits.py --record <commit>`", "groups": {}}
    for group, fn in GROUPS.items():
        arrays = fn(S)
        entries, parts, off = [], [], 0
        for key, a in arrays.items():
            a = np.asarray(a, dtype=np.float64)
            entries.append({"key": key, "shape": list(a.shape), "offset": off})
            parts.append(bits(a))
            off += a.size
        np.save(os.path.join(GOLDEN, f"{group}.npy"), np.concatenate(parts))
        manifest["groups"][group] = entries
        print(f"{group}: {len(entries)} arrays, {off * 8} bytes")
    with open(os.path.join(GOLDEN, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        record(sys.argv[2])
    else:
        raise SystemExit(__doc__)
