"""The backend-independent half of the C ABI (csrc/capi_shared.hpp) WITHOUT a GPU: the CPU harness of tests/cpu_engine
exports the very text libsabc_hip.so is built from, so what runs here -- null handles, the order of the hook setters, the
collectives' self-test and what it says about a transport that returns wrong words, the descriptor exchange of
sabc_comm_p2p_init(h, NULL), the host-staged round trip of device_buffers = 0 -- is the product's own C layer.
Shards are host threads of this process with in-process hooks (tests/test_p2p_cpu_engine.py: ThreadCollectives);
GaussianIID, 100 particles on 3 shards (34, 34, 32: the last shard's capacity is not its particle count), 3 updates."""
import ctypes as C

import numpy as np
import pytest

from tests.test_p2p_cpu_engine import ThreadCollectives, make_handle, run_shard_threads

CASE, ALG, N, WORLD, UPDATES = "gauss2_2stats", "multi_eps", 100, 3, 3
ERR_BAD_CONFIG, ERR_COMM, ERR_STATE = -8, -22, -23


class ThreadAllToAll(ThreadCollectives):
    """ThreadCollectives + the personalised exchange, and -- corrupt = "allreduce" | "allgather" | "alltoallv" -- hooks whose
    result has one word flipped on every shard (so that every shard's self-test ends at the same check)."""

    def __init__(self, world, corrupt=None):
        super().__init__(world)
        self.corrupt = corrupt

    def hooks(self, rank):
        W = self.world
        allreduce0, allgather0 = super().hooks(rank)

        def flip(ptr):
            w = C.c_uint64.from_address(ptr)
            w.value ^= 1 << 40                        # one bit of the mantissa: a finite, different double

        def view(ptr, n):                             # an empty side of an exchange may come with a null pointer
            return np.ctypeslib.as_array((C.c_double * n).from_address(ptr)) if n else np.zeros(0)

        def allreduce(ctx, buf, count, stream):
            rc = allreduce0(ctx, buf, count, stream)
            if self.corrupt == "allreduce":
                flip(buf)
            return rc

        def allgather(ctx, send, recv, count, stream):
            rc = allgather0(ctx, send, recv, count, stream)
            if self.corrupt == "allgather":
                flip(recv + 8 * count * (W - 1))      # the last shard's first word
            return rc

        def alltoallv(ctx, send, sc, recv, rc, nranks, stream):
            assert nranks == W
            sc, rc = [int(sc[p]) for p in range(W)], [int(rc[p]) for p in range(W)]
            self.slots[rank] = (view(send, sum(sc)).copy(), sc)
            self.barrier.wait()
            out = view(recv, sum(rc))
            o = 0
            for p in range(W):
                data, psc = self.slots[p]
                off = sum(psc[:rank])
                assert psc[rank] == rc[p]
                out[o:o + rc[p]] = data[off:off + rc[p]]
                o += rc[p]
            self.barrier.wait()
            if self.corrupt == "alltoallv":
                flip(recv)
            return 0

        return allreduce, allgather, alltoallv


def shard_threads(world, coll, body):
    """body(rank, barrier) per shard; a shard that fails releases the others from the hooks' barrier as well."""
    def guarded(rank, barrier):
        try:
            return body(rank, barrier)
        except BaseException:
            coll.barrier.abort()
            raise
    return run_shard_threads(world, guarded)


def install(h, coll, rank, device_buffers, alltoallv):
    ar, ag, a2a = coll.hooks(rank)
    h.set_collectives(ar, ag, device_buffers)
    if alltoallv:
        h.set_alltoallv(a2a)


def test_a_null_handle_gives_what_the_product_returns_function_by_function(S):
    """The table is capi.hip's as it stood before the entry points moved: SABC_ERR_STATE from what works on a handle,
    SABC_ERR_COMM from the hook setters, SABC_ERR_BAD_CONFIG from the two setters that check their argument in the same
    breath, 0 / 0.0 from the getters that return a number.  No crash."""
    from tests import cpu_engine
    L = cpu_engine.lib()
    dp = C.POINTER(C.c_double)
    d1, i4, i1, desc = (C.c_double * 64)(), (C.c_int64 * 4)(), C.c_int32(), C.create_string_buffer(S._lib.P2P_DESC_BYTES)
    ar = S._lib.ALLREDUCE_FN(lambda *a: 0)
    ag = S._lib.ALLGATHER_FN(lambda *a: 0)
    a2a = S._lib.ALLTOALLV_FN(lambda *a: 0)
    args = S._lib.UpdateArgs()
    p = C.cast(d1, dp)
    table = [
        ("sabc_set_collectives", (None, ar, ag, None, 0), ERR_COMM),
        ("sabc_set_alltoallv", (None, a2a), ERR_COMM),
        ("sabc_comm_bytes", (None,), 0),
        ("sabc_comm_selftest", (None,), ERR_STATE),
        ("sabc_initialize", (None, 1000), ERR_STATE),
        ("sabc_update", (None, C.byref(args)), ERR_STATE),
        ("sabc_n_global", (None,), 0),
        ("sabc_n_local", (None,), 0),
        ("sabc_local_offset", (None,), 0),
        ("sabc_get_population", (None, p, p, p), ERR_STATE),
        ("sabc_set_population", (None, p, p, p), ERR_STATE),
        ("sabc_get_counters", (None, i4), ERR_STATE),
        ("sabc_set_counters", (None, i4), ERR_STATE),
        ("sabc_get_epsilon", (None, p, C.byref(i1)), ERR_STATE),
        ("sabc_set_epsilon", (None, p, 1), ERR_STATE),
        ("sabc_history_len", (None,), 0),
        ("sabc_get_history", (None, p, p, p), ERR_STATE),
        ("sabc_clear_history", (None,), ERR_STATE),
        ("sabc_cdf_len", (None, 0), 0),
        ("sabc_get_cdf_knots", (None, 0, p), ERR_STATE),
        ("sabc_set_cdf_knots", (None, 0, p, 3), ERR_STATE),
        ("sabc_get_proposal_sigma", (None, p), ERR_STATE),
        ("sabc_last_ess", (None,), 0.0),
        ("sabc_host_syncs", (None,), 0),
        ("sabc_collective_calls", (None,), 0),
        ("sabc_persistent_launches", (None,), 0),
        ("sabc_persistent_lanes", (None,), 0),
        ("sabc_persistent_fallbacks", (None,), 0),
        ("sabc_comm_p2p_descriptor", (None, C.cast(desc, C.c_void_p)), ERR_STATE),
        ("sabc_comm_p2p_init", (None, None), ERR_STATE),
        ("sabc_comm_p2p_setup", (None,), ERR_STATE),
        ("sabc_comm_p2p_selftest", (None,), ERR_STATE),
        ("sabc_comm_p2p_set_timeout", (None, 100.0), ERR_BAD_CONFIG),
        ("sabc_comm_p2p_disable", (None,), ERR_STATE),
        ("sabc_comm_p2p_active", (None,), 0),
        ("sabc_comm_p2p_fallbacks", (None,), 0),
        ("sabc_comm_p2p_inject_silence", (None, 1), ERR_STATE),
        ("sabc_comm_p2p_inject_loss", (None, 1), ERR_STATE),
        ("sabc_comm_p2p_inject_stale", (None, 1), ERR_STATE),
        ("sabc_comm_p2p_set_destroy_wait", (None, 0.0), ERR_BAD_CONFIG),
    ]
    got = [(name, getattr(L, name)(*a)) for name, a, _ in table]
    assert got == [(name, want) for name, _, want in table]
    assert L.sabc_abi_version() == S._lib.ABI_VERSION
    # without a handle the handle's error text is the calling thread's global one
    assert L.sabc_last_error(None) == L.sabc_last_global_error()


def test_set_alltoallv_before_set_collectives_is_refused_in_the_products_words(S):
    coll = ThreadAllToAll(1)
    h = make_handle(S, CASE, ALG, N, 0, WORLD)
    a2a = coll.hooks(0)[2]
    with pytest.raises(S.SABCError, match="sabc_set_alltoallv needs the hooks of sabc_set_collectives to be installed first") as ei:
        h.set_alltoallv(a2a)
    assert ei.value.code == ERR_COMM
    h.close()


@pytest.mark.parametrize("device_buffers", [0, 1])
@pytest.mark.parametrize("alltoallv", [False, True])
def test_comm_selftest_passes_over_correct_hooks(S, device_buffers, alltoallv):
    coll = ThreadAllToAll(WORLD)

    def body(rank, barrier):
        h = make_handle(S, CASE, ALG, N, rank, WORLD)
        install(h, coll, rank, device_buffers, alltoallv)
        h.comm_selftest()
        calls = h.collective_calls              # the self-test talks to the hooks directly, not through the engine's counters
        h.close()
        return calls

    assert shard_threads(WORLD, coll, body) == [0] * WORLD


@pytest.mark.parametrize("device_buffers", [0, 1])
@pytest.mark.parametrize("corrupt,message", [("allgather", "self-test allgather gave wrong words"),
                                             ("allreduce", "self-test allreduce gave a wrong sum"),
                                             ("alltoallv", "self-test alltoallv gave wrong words")])
def test_comm_selftest_names_the_collective_that_returned_a_wrong_word(S, corrupt, message, device_buffers):
    coll = ThreadAllToAll(WORLD, corrupt=corrupt)

    def body(rank, barrier):
        h = make_handle(S, CASE, ALG, N, rank, WORLD)
        install(h, coll, rank, device_buffers, alltoallv=True)
        with pytest.raises(S.SABCError, match=message) as ei:
            h.comm_selftest()
        h.close()
        return ei.value.code

    assert shard_threads(WORLD, coll, body) == [ERR_COMM] * WORLD


def test_p2p_init_without_descriptors_gathers_them_over_the_collectives(S):
    coll = ThreadAllToAll(2)

    def body(rank, barrier):
        h = make_handle(S, CASE, ALG, N, rank, 2)
        install(h, coll, rank, 0, alltoallv=False)
        assert not h.p2p_active
        h.p2p_init(None)
        active = h.p2p_active
        barrier.wait()                          # nobody leaves while its peer may still be mapping it
        h.p2p_selftest()
        barrier.wait()
        h.close()
        return active

    assert shard_threads(2, coll, body) == [True, True]


def test_host_staging_is_the_same_run_as_backend_pointers(S):
    """device_buffers = 0 stages every allreduce, allgather and alltoallv through the collectives' host vector (to_host, the
    hook, to_backend); device_buffers = 1 hands the hooks the backend's own pointers.  Same words either way."""
    from tests.cases import MODELS, hip_proposal
    d = len(MODELS[CASE]["prior"])

    def run(device_buffers):
        coll = ThreadAllToAll(WORLD)

        def body(rank, barrier):
            h = make_handle(S, CASE, ALG, N, rank, WORLD)
            install(h, coll, rank, device_buffers, alltoallv=True)
            h.comm_selftest()
            h.initialize((UPDATES + 1) * N)
            for _ in range(UPDATES):
                h.update(n_simulation=N, proposal=hip_proposal(S, "de", d), resample=N // 4)
            res = dict(pop=h.get_population(), eps=h.eps, counters=h.counters, calls=h.collective_calls, comm=h.comm_bytes,
                       n_local=h.n_local)
            h.close()
            return res
        return shard_threads(WORLD, coll, body)

    staged, direct = run(0), run(1)
    assert [o["n_local"] for o in staged] == [34, 34, 32]
    assert staged[0]["counters"]["n_population_updates"] == UPDATES and staged[0]["counters"]["n_resampling"] >= 1
    for a, b in zip(staged, direct):
        for x, y in zip(a["pop"], b["pop"]):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(a["eps"], b["eps"])
        assert a["counters"] == b["counters"]
        assert a["calls"] == b["calls"] > 0 and a["comm"] == b["comm"] > 0


def test_the_c_abi_from_a_plain_program_two_shards_on_two_threads(tmp_path):
    """tests/cpu_engine/capi_probe.cpp, built plainly with the harness's own sources and flags: self-test over C hooks, then
    three updates; the shards end on bitwise the same epsilon and counters.  (The same program is what a sanitizer build of
    the C layer runs: nothing loaded into Python is instrumented.)"""
    import os
    import shutil
    import subprocess
    from tests import cpu_engine
    if not shutil.which("g++") or not shutil.which("gcc"):
        pytest.skip("g++ / gcc not found")
    probe, obj, exe = os.path.join(os.path.dirname(cpu_engine.__file__), "capi_probe.cpp"), str(tmp_path / "oracle.o"), str(tmp_path / "capi_probe")
    ref, eng, orc = cpu_engine._SRCS
    fp = ["-O1", "-fno-fast-math", "-ffp-contract=off"]
    r = subprocess.run(["gcc", "-std=c11", "-c", orc, "-o", obj] + fp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["g++", "-std=c++17", "-pthread", probe, ref, eng, obj, "-o", exe, "-lm"] + fp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("capi_probe ok"), (r.stdout, r.stderr[-2000:])
