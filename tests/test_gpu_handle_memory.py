"""What a handle owns in device and pinned memory goes back when it is closed.

Every allocation of the library is made by one of two owning types (csrc/device_buffer.hpp), which count the bytes they hold:
sabc_debug_live_bytes reports (device, pinned).  The counts must be above zero while a handle is open and back where they
started once it is closed -- for the one-launch form, the launch chain with a resample, host mode with a host prior, a
simulator from source, and the stand-alone operators, which own their temporaries for the length of one call.  A last case
does not use the counter at all: the device's free memory after repeated create / close cycles."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats

from tests.cases import SEED, hip_model_prior, hip_proposal
from tests.test_user_simulator import SHAPE_SRC, shape_params

pytestmark = pytest.mark.gpu


def live_bytes(S):
    out = (C.c_int64 * 2)()
    assert S.lib().sabc_debug_live_bytes(out) == 0
    return np.array([out[0], out[1]], dtype=np.int64)


def open_run_close(S, make_handle, n, prop, **upd):
    """create, initialize, two updates, close; returns (live bytes while open, after close) minus what was live before (other
    tests of the process may hold handles) and the counters at the end."""
    before = live_bytes(S)
    h = make_handle()
    try:
        h.initialize(4 * n)
        for _ in range(2):
            h.update(n_simulation=3 * n, proposal=prop, **upd)
        opened = live_bytes(S) - before
        counters = h.counters
    finally:
        h.close()
    return opened, live_bytes(S) - before, counters


def test_one_launch_form_returns_its_memory(S, gpu, monkeypatch):
    monkeypatch.delenv("SABC_PERSISTENT", raising=False)
    monkeypatch.delenv("SABC_PERSISTENT_MAX", raising=False)
    n = 1000
    model, prior = hip_model_prior(S, "gauss1_cfg2")
    before = live_bytes(S)
    h = S.SabcHandle(n_particles=n, model=model, prior=prior, seed=SEED)
    h.initialize(4 * n)
    h.update(n_simulation=3 * n, proposal=hip_proposal(S, "rw", 1))
    h.update(n_simulation=3 * n, proposal=hip_proposal(S, "rw", 1))
    assert h.persistent_launches >= 1                      # the grid barrier's words and the tagged rows are allocated
    opened = live_bytes(S) - before
    # the operators of a handle own their temporaries for one call only
    h.simulate(np.zeros((1, 1)), pid0=0, it=0)
    h.prior(0, 1)
    h.cdf_apply(np.ones((1, 1)))
    assert (live_bytes(S) - before == opened).all()
    h.close()
    assert opened[0] > 0 and opened[1] > 0
    assert (live_bytes(S) - before == 0).all()


def test_launch_chain_with_a_resample_returns_its_memory(S, gpu, monkeypatch):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    n = 4096
    model, prior = hip_model_prior(S, "gauss1_cfg2")
    opened, closed, counters = open_run_close(S, lambda: S.SabcHandle(n_particles=n, model=model, prior=prior, seed=SEED), n,
                                              hip_proposal(S, "de", 1), resample=n // 3)
    assert counters["n_resampling"] >= 1                   # the scan, pack and weight buffers were in use
    assert opened[0] > 0
    assert (closed == 0).all()


def test_host_mode_with_a_host_prior_returns_its_memory(S, gpu):
    n = 512
    rng = np.random.default_rng(SEED)
    model = S.HostDistance(lambda th: np.abs(th - 0.3), n_stats=1, n_para=1, univariate=True, batched=True)
    prior = S.HostPrior(lambda ids: rng.normal(0.0, 1.5, (len(ids), 1)), lambda th: stats.norm(0.0, 1.5).logpdf(th[:, 0]), 1)
    opened, closed, _ = open_run_close(S, lambda: S.SabcHandle(n_particles=n, model=model, prior=prior, seed=SEED), n,
                                       hip_proposal(S, "rw", 1))
    # every staging array of host mode is pinned: at least proposals, distances, current particles and two log densities per particle
    assert opened[0] > 0 and opened[1] >= 5 * n * 8
    assert (closed == 0).all()


def test_simulator_from_source_returns_its_memory(S, gpu):
    n, d, s = 1000, 2, 4
    model = S.DeviceSource(SHAPE_SRC, d, s, shape_params(d, s))
    prior = S.product_distribution([S.Normal(0.0, 1.0)] * d)
    opened, closed, _ = open_run_close(S, lambda: S.SabcHandle(n_particles=n, model=model, prior=prior, seed=SEED), n,
                                       S.RandomWalk(n_para=d))
    assert opened[0] > 0
    assert (closed == 0).all()


def test_stand_alone_operators_keep_nothing(S, gpu):
    before = live_bytes(S)
    calls = [lambda: S.op_sort([1.0]), lambda: S.op_build_cdf([1.0]), lambda: S.op_cdf_eval([0.0, 1.0], [0.5]),
             lambda: S.op_philox(0, 0, 0, 0, 0), lambda: S.op_normal_pairs(SEED, 0, 1), lambda: S.op_rng_peak(1, 1, 1)]
    for call in calls:
        call()
        assert (live_bytes(S) - before == 0).all()
    with pytest.raises(S.SABCError):                       # an operator that fails gives its temporaries back as well
        S.op_build_cdf([1.0, -0.5, 2.0])
    assert (live_bytes(S) - before == 0).all()


def test_free_device_memory_does_not_shrink_over_create_close_cycles(S, gpu, monkeypatch):
    """gauss1_cfg2, RandomWalk, the launch chain, n = 200 000: each population buffer is 3 x 200 000 x 8 B = 4.8 MB.  After a
    warm-up cycle, five more cycles of create / initialize / update / close must not leave the device with a population
    buffer's worth less free memory -- a bound from the shapes, which holds with or without the owning types."""
    import torch
    torch.cuda.mem_get_info()                              # (torch sets itself up on the device at its first call: not a cycle's doing)
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    n = 200_000
    model, prior = hip_model_prior(S, "gauss1_cfg2")

    def cycle():
        h = S.SabcHandle(n_particles=n, model=model, prior=prior, seed=SEED)
        h.initialize(2 * n)
        h.update(n_simulation=n, proposal=hip_proposal(S, "rw", 1))
        h.close()
    cycle()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(5):
        cycle()
    free1 = torch.cuda.mem_get_info()[0]
    print(f"free device memory: {free0} -> {free1} ({free0 - free1:+d} B used)")
    assert free0 - free1 < 3 * n * 8
