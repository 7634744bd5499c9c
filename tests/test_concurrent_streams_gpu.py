"""One plan shared by concurrent streams and by host threads (include/grbda_hip.h: a plan "is immutable after creation and may be shared
by threads and streams"): a call's result must be BIT-identical whether or not other calls of the same plan are in flight, and the
result it is compared with -- the same call made alone -- is itself held against the oracle.  concurrency.py gives the gate, the
round-robin enqueue, the per-repetition events and the overlap count.

1. Every row of the entry-point table (entry_points.py: the inverse-dynamics derivatives, integrate / step / rollout, the contact entry
   points, energy, the centroidal quantities and the momentum matrix included), fp32 and fp64, on N_STREAMS = 4 streams.  Stream i has its own inputs (seed
   100 + i) and its own batch B - i, so the streams are ragged differently and hold slabs of different sizes on the row's route.
   Serial pass: one call per stream, alone, against the oracle on edge_states(B - i).  Concurrent pass: behind a gate (a spin kernel all
   worker streams wait for) the host queues R repetitions round-robin over the streams, every repetition into fresh outputs.  Asserted:
   the gate was still closed when the last call had been queued; every output of every repetition (integer outputs included) has the
   serial bits; every input has the bits it had; and two repetitions on different streams have intersecting event windows.
2. Cold start: a FRESH plan per kind of per-stream state makes its first calls in the gated concurrent pass, so that every stream's
   slab is allocated while the other streams' calls are queued or running (gated(): what the gate can and cannot hold back there);
   the serial pass follows.  Also the minv derivatives capped to 1 MiB of work slab at 20 000 fp32 states: many-chunk calls of four
   streams interleaved.
3. Host threads: the rows of 2, four threads with a stream each, released by a barrier, R calls each.  Two threads on ONE stream of a
   fresh plan, one repeating a small batch while the other walks a ladder of growing batches (every step frees and reallocates that
   stream's slab): the situation the comment on grbda_plan::mu describes.  A refused call in one thread (device index out of range)
   leaves its text in that thread's grbda_last_error() and the other thread's results, and both threads' HIP device, alone.
4. Two plans alternating on one stream (slabs are per plan), and grbda_plan_release_work() called with calls queued behind the gate.

The tests set no runtime option and read no environment beyond the plan-time switches of the table and GRBDA_WORK_MAX_MB."""
import ctypes
import time

import numpy as np
import pytest

import concurrency as C
import generalized_rbda_amd as G
from entry_points import CASES, ENTRY, IDS, NOT_RUN, TOL32, TOL64, TYPED, TYPED_IDS, _host, _inputs, _model, draw_bound, edge_states, plan_for, same_bits_np

pytestmark = pytest.mark.gpu

N_STREAMS = C.N_STREAMS
R = 8
SEED0 = 100


def _dtype(name):
    import torch

    return torch.float64 if name == "f64" else torch.float32


_streams = None


def _workers():
    """the worker streams, made once: a warm plan then keeps one slab per worker, a fresh plan has seen none of them"""
    global _streams
    if _streams is None:
        import torch

        _streams = [torch.cuda.Stream() for _ in range(N_STREAMS)]
    return _streams


def _fresh_plan(model, env):
    """a new plan under the row's switches (plan_for without its cache)"""
    return plan_for.__wrapped__(model, tuple(sorted(env.items())))


def _check_route(plan, route, entry, dtype_name, sizes):
    """the row's route at every stream's batch size, as test_graph_capture_gpu.py checks it at the row's own"""
    if entry in ("aba", "rnea"):
        want = {"chain": "_chain_kernel<", "latency": "_chain_lm_kernel<", "interpreter": f"{entry}_kernel<", "gen1": "_gen1_kernel<"}.get(route)
        for b in sizes:
            name = plan.kernel_name(entry, dtype_name, b)
            assert want is None or (want in name and ("_lm_kernel<" in name) == (route == "latency")), (b, name)
    if route in ("spanning_tree", "two_parent"):
        assert plan.info().spanning_tree_route == 1


class _Streams:
    """The inputs of one case on the worker streams and the three passes over them."""

    def __init__(self, plan, model, entry, dtype_name, gpu, sizes, seed0=SEED0):
        import torch

        self.plan, self.blob, self.entry, self.gpu = plan, _model(model), entry, gpu
        self.call, self.check = ENTRY[entry]
        self.tol = TOL64 if dtype_name == "f64" else TOL32
        self.streams = _workers()[:len(sizes)]
        self.sizes = list(sizes)
        self.s, self.x = [], []
        for i, b in enumerate(sizes):
            s, x = _inputs(self.blob, plan, b, seed0 + i, _dtype(dtype_name), gpu, draw_bound(entry))
            self.s.append(s)
            self.x.append(x)
        self.before = [{k: v.clone() for k, v in x.items() if k != "q_proj"} for x in self.x]
        torch.cuda.synchronize()

    def one(self, plan, i):
        """stream i's call with the current stream; project_positions works in place, so every call gets its own copy of q_start"""
        return self.call(plan, {**self.x[i], "q_proj": self.x[i]["q_start"].clone()})

    def serial(self, plan=None, oracle=True):
        """each stream's call alone: (outputs per stream, host seconds the calls took to enqueue)"""
        plan = plan or self.plan
        import torch

        outs, t_enqueue = [], 0.0
        for i, st in enumerate(self.streams):
            with torch.cuda.stream(st):
                t0 = time.perf_counter()
                o = self.one(plan, i)
                t_enqueue += time.perf_counter() - t0
            st.synchronize()
            outs.append(tuple(o))
            if oracle and self.check is not None:
                idx = edge_states(self.sizes[i], seed=self.sizes[i])
                host = _host(o)
                assert all(len(h) == self.sizes[i] for h in host)
                self.check(self.blob, {k: v[idx] for k, v in self.s[i].items()}, [h[idx] for h in host], self.tol)
        return outs, t_enqueue

    def gated(self, t_enqueue, reps=R, cold=False):
        """R repetitions per stream queued round-robin behind a gate sized from `t_enqueue`; returns outs[i][r].  Asserted: the gate was
        still closed when the last call had been queued, and two calls on different streams have intersecting event windows.

        cold: every worker stream's first call of a fresh plan (whose tables another stream has uploaded: cold_start_case).  The gate
        cannot always outlast those.  Growing a slab frees the old one first, hipFree waits for every stream of the device -- the
        gate's included -- and a first call that sizes its stream's slab twice (the derivatives: the forward dynamics' share, then
        the recursion's) frees what it has just allocated; other allocations of the runtime may wait as well.  The host then sits
        inside that call until the gate opens, however long the gate is, and leaves it with the device nearly idle.  On the MI355X
        this was always the FIRST call of the pass, and not in the same rows from one run to the next.  That cannot be undone from
        outside the library, and the test does not pretend otherwise.  Asserted of a cold pass:
          * where the gate outlasted the enqueue: every stream's first call was issued beside incomplete work of another stream, and
            the FIRST calls of two streams have intersecting windows;
          * where it did not: the gate was closed at the start of every call up to the one in which it opened (the trace of
            round_robin), and without that one call's duration the whole enqueue fits into the gate -- the host waited in ONE call, it
            was not slow everywhere behind a gate that was too short -- and at least one stream's first call was issued beside
            incomplete work of another stream;
          * in both: over all repetitions, calls on two streams overlapped."""
        plan = self.plan
        import torch

        n = len(self.streams)
        gate = C.Gate(C.gate_ms(t_enqueue, reps))
        gate.hold(self.streams)
        t0 = time.perf_counter()
        outs, events, trace = C.round_robin(self.streams, [lambda r, i=i: tuple(self.one(plan, i)) for i in range(n)], reps, gate)
        held = gate.held()
        t_queue = time.perf_counter() - t0
        torch.cuda.synchronize()
        win = C.windows(gate.origin, events)
        pairs, pairs0 = C.overlapping(win), C.overlapping([per[:1] for per in win])
        n_held = sum(1 for rec in trace if rec[3])
        waited = trace[n_held - 1][5] - trace[n_held - 1][2] if 0 < n_held else 0.0  # (the call during which the gate opened)
        busy_first = [rec[4] for rec in trace if rec[1] == 0 and rec[0] > 0]
        self.report = (f"gate {gate.ms:.2f} ms asked, {gate.origin.elapsed_time(gate.opened):.2f} ms run (serial enqueue {t_enqueue * 1e3:.3f} ms); "
                       f"{reps} x {n} calls queued in {t_queue * 1e3:.2f} ms, gate closed at the end: {held}, at the start of the first {n_held} "
                       f"calls, {waited * 1e3:.2f} ms spent in the last of those; first calls issued beside incomplete work: {busy_first}; "
                       f"first-call windows {[tuple(round(t, 3) for t in per[0]) for per in win]} ms; overlapping pairs: {pairs0} among first calls, "
                       f"{pairs} in all")
        if not cold:
            assert held, "the gate opened before the last call was queued: " + self.report
        elif not held:
            assert n_held > 0 and all(rec[3] for rec in trace[:n_held]) and (t_queue - waited) * 1e3 < gate.ms, \
                "the gate opened during the enqueue, and not because the host waited for it inside one call: " + self.report
        assert not cold or (all(busy_first) if held else any(busy_first)), \
            "first calls were issued with nothing of the other streams queued or running: " + self.report
        assert not (cold and held) or pairs0 > 0, "no two first calls were in flight at the same time: " + self.report
        assert pairs > 0, "no two calls on different streams were in flight at the same time: " + self.report
        return outs

    def assert_same(self, outs, serial, what):
        """outs[i] = one output tuple or a list of them; all equal to serial[i] bit for bit, and the inputs untouched"""
        for i, per in enumerate(outs):
            for r, o in enumerate(per if isinstance(per, list) else [per]):
                assert C.same_bits(o, serial[i]), f"{what}: stream {i} (B = {self.sizes[i]}), repetition {r} differs from the serial call" + _where(o, serial[i])
        self.assert_inputs_untouched()

    def assert_inputs_untouched(self):
        for i, keep in enumerate(self.before):
            for k, v in keep.items():
                assert C.same_bits(self.x[i][k], v), f"input {k} of stream {i} changed"


def _where(got, want):
    """which states differ, for the message of a failed comparison"""
    out = ""
    for n, (a, b) in enumerate(zip(_host(got), _host(want))):
        if a.shape == b.shape and not same_bits_np([a], [b]):
            bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
            out += f"; output {n}: {len(bad)} of {len(a)} states, first {bad[:8]}, max |diff| {np.nanmax(np.abs(a.astype(float) - b.astype(float))):.3e}"
    return out


# ---- 1. streams sharing a plan give the serial bits ------------------------------------------------------------------------------------
SHARED, SHARED_IDS = TYPED, TYPED_IDS
# every row of the table, both types, less what the table itself leaves out
assert {i.rsplit("-", 1)[0] for i in SHARED_IDS} == set(IDS) and len(SHARED) == 2 * len(CASES) - len(NOT_RUN)


def shared_plan_case(case, dtype_name, gpu, sizes=None):
    route, model, env, B, entry = case
    plan = plan_for(model, tuple(sorted(env.items())))
    sizes = sizes or [B - i for i in range(N_STREAMS)]
    _check_route(plan, route, entry, dtype_name, sizes)
    w = _Streams(plan, model, entry, dtype_name, gpu, sizes)
    serial, t_enqueue = w.serial()
    w.assert_same(w.gated(t_enqueue), serial, "concurrent pass")
    again, _ = w.serial(oracle=False)  # (and the serial call is reproducible with nothing else in flight)
    w.assert_same(again, serial, "second serial pass")


@pytest.mark.parametrize("case,dtype_name", SHARED, ids=SHARED_IDS)
def test_streams_sharing_a_plan_give_the_serial_bits(case, dtype_name, gpu):
    shared_plan_case(case, dtype_name, gpu)


# ---- 2. cold start ---------------------------------------------------------------------------------------------------------------------
def _row(route, model, entry, B=None):
    rows = [c for c in CASES if c[0] == route and c[1] == model and c[4] == entry and (B is None or c[3] == B)]
    assert len(rows) == 1, (route, model, entry, rows)
    return rows[0]


# one row per kind of per-stream state: (what the row's streams own, row of the table, types)
STATE_ROWS = [
    ("scratch slab", _row("interpreter", "urdf_mit_humanoid", "aba"), ("f64", "f32")),
    ("split layout, [K | y0] blocks in the global slab", _row("chain", "urdf_mini_cheetah", "aba"), ("f32",)),
    ("work", _row("no_crba", "urdf_mini_cheetah", "mass_matrix"), ("f64", "f32")),
    ("work_cvt, projection", _row("manifold", "urdf_four_bar", "fd_dq"), ("f32",)),
    ("deriv_chunk (minv)", _row("minv", "urdf_mini_cheetah", "fd_derivatives"), ("f64", "f32")),
    ("deriv_chunk (dense)", _row("dense", "urdf_mini_cheetah", "fd_derivatives"), ("f64", "f32")),
    ("deriv_chunk, the span sub-plan", _row("manifold", "tello", "fd_derivatives"), ("f64", "f32")),
    ("zero block", _row("chain", "urdf_mini_cheetah", "inv_osim"), ("f64", "f32")),
    ("work_proj (forward dynamics)", _row("spanning_tree", "parallel_chain_exp_d10_l16", "aba"), ("f64", "f32")),
    ("work_proj (mass matrix)", _row("spanning_tree", "parallel_chain_exp_d10_l16", "mass_matrix"), ("f64", "f32")),
    ("scratch slab of the auxiliary kernels", _row("implicit", "urdf_four_bar", "project_positions"), ("f64", "f32")),
    ("parents' pose, velocity and acceleration rows of centroidal_kernel in the scratch slab", _row("explicit", "urdf_mit_humanoid", "centroidal"), ("f64", "f32")),
    ("work slab of the contact pipeline", _row("efpa", "urdf_mini_cheetah", "contact_dynamics"), ("f64", "f32")),
    ("work slab of the momentum matrix", _row("explicit", "urdf_mit_humanoid", "centroidal_matrix"), ("f64", "f32")),
    ("forward dynamics and projection chained on one stream", _row("explicit", "urdf_mini_cheetah", "rollout"), ("f64", "f32")),
]
# the minv derivatives under GRBDA_WORK_MAX_MB=1 at the batch test_graph_capture_gpu.py captures: many chunks per call
CAPPED = ("chunked: 1 MiB of work slab", ("minv", "urdf_mini_cheetah", {}, 20000, "fd_derivatives"), ("f32",))
STATES = [(what, case, dt, 0) for what, case, dts in STATE_ROWS for dt in dts] + [(CAPPED[0], CAPPED[1], "f32", 1)]
STATES_IDS = [f"{c[4]}-{c[0]}-{c[1]}-B{c[3]}-{dt}" + ("-capped" if cap else "") for _, c, dt, cap in STATES]


def _cap(monkeypatch, cap_mb):
    if cap_mb:
        monkeypatch.setenv("GRBDA_WORK_MAX_MB", str(cap_mb))


def cold_start_case(what, case, dtype_name, gpu):
    route, model, env, B, entry = case
    sizes = [B - i for i in range(N_STREAMS)]
    pilot = _fresh_plan(model, env)
    _check_route(pilot, route, entry, dtype_name, sizes)
    w = _Streams(pilot, model, entry, dtype_name, gpu, sizes)
    _, t_enqueue = w.serial(oracle=False)
    del pilot
    plan = w.plan = _fresh_plan(model, env)
    # (the plan's tables go to the device in its first call, with synchronous copies that are no per-stream state: made here on a stream
    # of its own, so that the worker streams' first calls are left with what is theirs -- their slabs)
    import torch

    with torch.cuda.stream(torch.cuda.Stream()):
        w.one(plan, 0)
    torch.cuda.synchronize()
    cold = w.gated(t_enqueue, cold=True)
    serial, _ = w.serial()
    w.assert_same(cold, serial, f"cold concurrent pass ({what})")


@pytest.mark.parametrize("what,case,dtype_name,cap_mb", STATES, ids=STATES_IDS)
def test_cold_start_while_other_streams_run(what, case, dtype_name, cap_mb, gpu, monkeypatch):
    """A fresh plan's first calls on the worker streams, four streams at once.  The gate is sized from the first calls of ANOTHER fresh plan of the same row
    (made alone, stream after stream), which pay for the table upload and the allocations as the measured calls will."""
    _cap(monkeypatch, cap_mb)
    cold_start_case(what, case, dtype_name, gpu)


# ---- 3. host threads -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,case,dtype_name,cap_mb", STATES, ids=STATES_IDS)
def test_host_threads_sharing_a_plan(what, case, dtype_name, cap_mb, gpu, monkeypatch):
    import torch

    route, model, env, B, entry = case
    _cap(monkeypatch, cap_mb)
    plan = _fresh_plan(model, env) if cap_mb else plan_for(model, tuple(sorted(env.items())))  # (the capped slabs: not in the shared plan)
    w = _Streams(plan, model, entry, dtype_name, gpu, [B - i for i in range(N_STREAMS)])
    serial, t_enqueue = w.serial()  # (warm: every stream holds its slab)
    # (behind a gate, so that the threads' calls meet on the device as well as on the plan's mutex; whether the gate outlasts the four
    # threads' enqueue is not asserted here, the overlap is)
    gate = C.Gate(C.gate_ms(t_enqueue, R))
    gate.hold(w.streams)

    def body(i):
        def run():
            outs, events = [], []
            with torch.cuda.stream(w.streams[i]):
                for _ in range(R):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    outs.append(tuple(w.one(plan, i)))
                    b.record()
                    events.append((a, b))
            w.streams[i].synchronize()
            return outs, events
        return run

    got = C.in_threads([body(i) for i in range(N_STREAMS)])
    torch.cuda.synchronize()
    win = C.windows(gate.origin, [events for _, events in got])
    assert C.overlapping(win) > 0, f"no two threads' calls were in flight at the same time: windows {win}"
    w.assert_same([outs for outs, _ in got], serial, f"host threads ({what})")


# thread B's ladder: every step needs a larger slab on the stream than the one before.  The interpreter's slab follows its persistent
# grid, min(tiles, n_cu x wavefronts per CU) with at least four wavefronts per CU (the test asserts that the ladder stays below that);
# the derivatives' work slab is linear in the batch (the test reads its size back after every step of a dry ladder)
GROWING = {
    "interpreter_aba": (_row("interpreter", "urdf_mit_humanoid", "aba"), 200, [300, 2000, 8000, 4 * 4096 + 3, 40000]),
    "dense_derivatives": (_row("dense", "urdf_mini_cheetah", "fd_derivatives"), 65, [130, 301, 1001, 3002, 6003]),
}


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("name", list(GROWING))
def test_two_threads_one_stream_growing_slab(name, dtype_name, gpu):
    """Thread A repeats a small batch on stream s while thread B walks a ladder of growing batches on the same s of a fresh plan: B's
    hipFree of the slab A's kernels use may only come behind A's launches (grbda_plan::mu is held until a call's last kernel is
    enqueued, and hipFree waits for the stream).  B takes its next step only after A has begun two more calls, and A goes on until B
    is done, so A calls at every size of the slab: asserted from the step A saw at the start of each of its calls."""
    import threading

    import torch

    (route, model, env, _, entry), B_small, ladder = GROWING[name]
    sizes = [B_small] + ladder
    w = _Streams(plan_for(model, tuple(sorted(env.items()))), model, entry, dtype_name, gpu, sizes, seed0=200)
    w.streams = [_workers()[0]] * len(sizes)  # (one stream for all of them)
    serial, _ = w.serial()
    st = _workers()[1]
    # every step grows the slab
    tiles = [(b + 63) // 64 for b in sizes]
    assert tiles == sorted(set(tiles))
    if entry == "aba":
        assert tiles[-1] <= 4 * torch.cuda.get_device_properties(gpu).multi_processor_count, "the ladder's top is beyond the persistent grid"
    else:
        dry, held = _fresh_plan(model, env), []
        with torch.cuda.stream(st):
            for k in range(len(sizes)):
                w.one(dry, k)
                st.synchronize()
                held.append(dry.release_work())
        assert all(x < y for x, y in zip(held, held[1:])) and held[0] > 0, held
        del dry
    plan = _fresh_plan(model, env)
    done, begun, step = threading.Event(), [0], [0]
    LIMIT = 100 * R

    def small():
        outs, seen = [], []
        with torch.cuda.stream(st):
            while len(outs) < LIMIT and not (done.is_set() and len(outs) >= R):
                seen.append(step[0])
                begun[0] += 1
                outs.append(tuple(w.one(plan, 0)))
        return outs, seen

    def growing():
        outs = []
        try:
            with torch.cuda.stream(st):
                for k in range(len(ladder)):
                    outs.append(tuple(w.one(plan, 1 + k)))
                    step[0] = k + 1
                    at, t_end = begun[0], time.perf_counter() + 30.0
                    while begun[0] < at + 2 and begun[0] < LIMIT and time.perf_counter() < t_end:
                        time.sleep(0)
            return outs
        finally:
            done.set()

    (a, seen), b = C.in_threads([small, growing])
    torch.cuda.synchronize()
    assert set(seen) >= set(range(1, len(ladder) + 1)), f"thread A's {len(a)} calls began at steps {sorted(set(seen))} of thread B's {len(ladder)}"
    w.assert_same([a] + b, serial, "two threads on one stream")


def test_error_text_stays_with_its_thread(gpu):
    """Thread A's calls are refused on the host (device index out of range, GRBDA_EINVAL) while thread B's succeed: A reads the text of
    its own refusal and its output is not written, B's results are the serial bits and B has no error text, and the current HIP device
    of both threads is what it was."""
    import torch

    from graph_capture import hip_runtime

    L, hip = G.lib(), hip_runtime()
    plan = plan_for("urdf_mini_cheetah", ())
    w = _Streams(plan, "urdf_mini_cheetah", "aba", "f64", gpu, [1000, 300])
    serial, _ = w.serial()
    canary = torch.full((300, plan.nv), -7.0, dtype=torch.float64, device=gpu)
    torch.cuda.synchronize()
    bad_device = G.device_count() + 3

    def current_device():
        d = ctypes.c_int(-1)
        assert hip.hipGetDevice(ctypes.byref(d)) == 0
        return d.value

    def refused():
        x, seen = w.x[1], []
        before = current_device()
        for _ in range(4 * R):
            rc = L.grbda_aba_f64(plan._h, x["q"].data_ptr(), x["qd"].data_ptr(), x["tau"].data_ptr(), None, canary.data_ptr(), 300, bad_device,
                                 ctypes.c_void_p(w.streams[1].cuda_stream))
            seen.append((rc, (L.grbda_last_error() or b"").decode()))
        return seen, before, current_device()

    def succeeding():
        before = current_device()
        with torch.cuda.stream(w.streams[0]):
            outs = [tuple(w.one(plan, 0)) for _ in range(4 * R)]
        w.streams[0].synchronize()
        return outs, (L.grbda_last_error() or b"").decode(), before, current_device()

    (seen, a_before, a_after), (outs, b_text, b_before, b_after) = C.in_threads([refused, succeeding])
    torch.cuda.synchronize()
    assert all(rc == -1 and "device index out of range" in text for rc, text in seen), seen[:3]  # GRBDA_EINVAL
    assert b_text == "", b_text
    assert a_before == a_after == b_before == b_after == torch.cuda.current_device()
    assert bool((canary == -7.0).all()), "a refused call wrote to its output"
    w.assert_same([outs], serial[:1], "calls beside a refused one")


# ---- 4. two plans on one stream; release_work with work in flight ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("entry", ["aba", "rnea", "fd_derivatives"])
def test_two_plans_alternate_on_one_stream(entry, dtype_name, gpu):
    """Mini Cheetah and the four-bar in turn on one stream: slabs are per plan, so each gives what it gives alone."""
    import torch

    models = ("urdf_mini_cheetah", "urdf_four_bar")
    st = _workers()[0]
    ws = [_Streams(plan_for(m, ()), m, entry, dtype_name, gpu, [1000 - k], seed0=300 + k) for k, m in enumerate(models)]
    for w in ws:
        w.streams = [st]
    alone = [w.serial()[0][0] for w in ws]
    with torch.cuda.stream(st):
        outs = [[tuple(w.one(w.plan, 0)) for w in ws] for _ in range(R)]
    st.synchronize()
    for k, w in enumerate(ws):
        w.assert_same([[o[k] for o in outs]], [alone[k]], f"{models[k]} alternating with {models[1 - k]}")


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_release_work_with_work_in_flight(dtype_name, gpu):
    """R derivative calls queued behind the gate on one stream, grbda_plan_release_work() called at once: it waits for them (hipFree),
    hands the slab back, the results are the serial bits, and the next call on the stream allocates again."""
    import torch

    route, model, env, B, entry = _row("minv", "urdf_mini_cheetah", "fd_derivatives")
    plan = _fresh_plan(model, env)
    w = _Streams(plan, model, entry, dtype_name, gpu, [B])
    serial, t_enqueue = w.serial()
    gate = C.Gate(C.gate_ms(t_enqueue, R))
    gate.hold(w.streams)
    with torch.cuda.stream(w.streams[0]):
        outs = [tuple(w.one(plan, 0)) for _ in range(R)]
    assert gate.held(), "the calls had started before release_work was called"
    released = plan.release_work()
    torch.cuda.synchronize()
    assert released > 0
    assert plan.release_work() == 0  # (nothing is held now)
    w.assert_same([outs], serial, "calls whose work slab was released behind them")
    again, _ = w.serial(oracle=False)
    w.assert_same(again, serial, "the call after release_work")
    assert plan.release_work() > 0  # (it had allocated again)
