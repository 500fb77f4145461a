"""Stream ordering (GPU): every device-side entry of include/lorastencil.h is "asynchronous on `stream`" -- all the work a call
enqueues (halo copies, resets and wraps, the copies in and out of the ghost-extended periodic grid, launches through plan-owned
grids, a captured graph, probes and record read-backs) is ordered on the caller's stream and on nothing else.  On an idle device
work put on the wrong stream still runs in program order, so every other test passes whether that holds or not.  Here a GATE --
``torch.cuda._sleep``: one workgroup spinning for a bounded, calibrated time -- is queued in front of the call, so that work on
the wrong stream runs visibly at the wrong time:

  A  the gate on the caller's stream S, then on S the uploads of the real input over grids full of tests/arena.py's poison, the
     call, a copy of every whole arena (guard bands included) into a snapshot, poison again.  Library work that is not ordered
     on S runs before the input exists: the snapshot carries poison or stale halos.
  B  the gate on the null stream, the same sequence on S.  Library work left on the null stream runs late, on top of the poison
     S has put back: after the device has drained every grid must still hold nothing but poison.

What a snapshot must equal is the same call, ungated, on an idle and synchronised device by a fresh plan of the same
configuration: bit for bit, the whole padded arrays of every buffer (the kernels are deterministic; the ungated results are
pinned to the oracle by the other GPU tests).

Conditions asserted besides the bits, without which a pass proves nothing: the PREMISE (while the gate is pending on one stream
a copy on another one completes -- else the two share a hardware queue and the module fails, loudly), once when the streams are
picked and once more by EVERY gated call for itself, before its bits are judged (Ctx.gated, require_case_premise: the streams
were still served independently while this case's gate was pending, and the host was not held up past the gate); after a non-blocking
entry returns the gated stream is still busy (in A: the call did not wait for its own stream; in B: not for the null stream);
the entries documented as blocking (stats, diff, residual, residual_src, run_until, run_chebyshev_until) have drained S when
they return in A, and return while the null stream's gate is pending in B -- they wait for `stream`, not for the device; one
NEGATIVE CONTROL per scenario (the call handed another stream than the one that carries the gated uploads) does NOT match.

Gate length: the host time of the same call, ungated, on a warm plan is measured per case; G = max(50 ms, 10 x that), at most
500 ms.  COLD: first-need allocations (scratch grid, leapfrog grids, probe grid, records, extended periodic grids) happen inside
the gated call: the result alone is asserted.  PREPARED: ``prepare_run`` was called, or the plan has made one such run, before
the gate: the result and that the call did not block.  Kernel code objects are loaded per process, so the reference run of a
twin plan warms them first.  Nothing is allocated or freed while a gate is pending; every plan lives until its case has drained.
Every stream has run something before its first gate: the FIRST use of a stream sets up its queue, and that waited for a gate
pending on another stream (measured: the premise of A failed with a second stream first used behind S's gate, and held once
every stream had been used before).  Streams that share one of the process's four hardware queues are served one behind the
other whatever the code does; Ctx._pick_streams draws streams until two are independent of the null stream and of each other.

One case turns scenario B round: a cold run that is still in flight when the null stream's gate runs out
(test_a_cold_run_still_in_flight_...), which is where work left on the null stream lands in the middle of the run.
"""
import dataclasses
import time

import numpy as np
import pytest

import arena as A
from test_gpu_leapfrog_src import RUNS, host_data, real_taps
from test_gpu_memory_contract import ROW_IDS, ROWS, _input, _make_plan

pytestmark = pytest.mark.gpu

GATE_MIN_MS, GATE_MAX_MS, GATE_FACTOR = 50.0, 500.0, 10.0
SCENARIOS = ("A", "B")
RHO = 0.9
UNTIL = dict(tol=1e-12, rtol=0.0, check_every=4, max_times=8)


# ---------------------------------------------------------------------------------------------------------------------------
# the gate, the premise, the gated call
# ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Job:
    """One call under test: its grids, what is uploaded into them behind the gate, and the call itself."""
    kind: str                      # what the host-time / gate-length report files it under
    arenas: list                   # every buffer the call may read or write, carved out of poisoned allocations
    uploads: list                  # [(integer view of a grid, staged integer tensor of its input)]
    make_plan: object              # () -> a fresh plan of the configuration
    call: object                   # (plan, stream) -> what the entry returns (None for the launches and runs)
    prepare: object = None         # (plan) -> None: the entry's prepare call; None: one ungated call of the same kind
    blocking: bool = False         # the entry is documented to block until its result is on the host
    snaps: list = None             # one tensor per arena, made while the device was idle

    def __post_init__(self):
        import torch

        self.snaps = [torch.empty_like(ar.flat) for ar in self.arenas]


@dataclasses.dataclass
class Ref:
    plan: object       # (kept: its grids are freed with it, and hipFree synchronises the device)
    ret: object
    expected: list     # the arenas' bits after the ungated call
    host_ms: float
    gate_ms: float
    job: object        # the Job it was made with: its buffers are the ones every case of the configuration runs on


@dataclasses.dataclass
class Gated:
    ret: object
    busy_after: bool        # the gated stream had not drained when the call returned
    drained_after: bool     # S had drained when the call returned
    host_ms: float
    clean: bool             # after everything drained, every arena held nothing but poison
    premise: object         # THIS case's premise: work on the ungated stream completed while the gate was pending (None: not asked)


class Ctx:
    def __init__(self, L, O):
        import torch

        self.torch, self.L, self.O = torch, L, O
        self.NULL = torch.cuda.default_stream()
        self.tiny = (torch.arange(64, dtype=torch.int64, device="cuda"), torch.zeros(64, dtype=torch.int64, device="cuda"))
        torch.cuda.synchronize()
        self.cycles_per_ms = self._calibrate()
        self.gate_50_ms = self._timed_gate(50.0)
        self.done = torch.cuda.Event()
        self.S, self.T, self.premise = self._pick_streams()
        self.report = {}   # kind -> [host ms (min, max), gate ms (min, max), cases]
        self.refs = {}
        print(f"\nstream-order: {self.cycles_per_ms:.0f} cycles per ms; a 50 ms gate lasted {self.gate_50_ms:.1f} ms; "
              f"premise {self.premise}")

    # -- the gate
    def _timed_sleep(self, cycles):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(int(cycles))
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def _calibrate(self):
        self._timed_sleep(1000)  # (the spin kernel's code object)
        cycles = 10_000_000
        ms = self._timed_sleep(cycles)
        if ms < 20.0:  # a fast counter: a longer spin for the same precision
            cycles = int(cycles * 40.0 / max(ms, 0.01))
            ms = self._timed_sleep(cycles)
        assert 1.0 < ms < 2000.0, f"torch.cuda._sleep({cycles}) took {ms} ms: not a usable gate"
        return cycles / ms

    def _timed_gate(self, ms):
        return self._timed_sleep(ms * self.cycles_per_ms)

    def gate(self, stream, ms):
        with self.torch.cuda.stream(stream):
            self.torch.cuda._sleep(int(ms * self.cycles_per_ms))

    def _passes(self, gated, other):
        """While a gate is pending on `gated`, a tiny copy on `other` completes: an event recorded behind the copy is reached,
        and ``other.synchronize()`` returns, while ``gated.query()`` is still false and within a quarter of the gate's length.
        Bounded either way: at the latest the waits return when the gate has run out.  Returns (passed, host ms of the waits)."""
        torch = self.torch
        torch.cuda.synchronize()
        done = torch.cuda.Event()
        self.gate(gated, GATE_MIN_MS)
        t0 = time.perf_counter()
        with torch.cuda.stream(other):
            self.tiny[1].copy_(self.tiny[0])
            done.record()
        done.synchronize()
        reached = not gated.query()
        other.synchronize()
        returned = not gated.query()
        ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        if reached != returned:
            print(f"\nstream-order premise: event reached while gated: {reached}, synchronize() returned while gated: {returned}")
        # (the waits must also have returned EARLY: a wait that returns just as the gate runs out can still find query() false)
        return reached and returned and ms < GATE_MIN_MS / 4, ms

    def _pick_streams(self):
        """S (the caller's stream) and T (the negative control's): two of torch's side streams -- non-blocking, as every
        ``torch.cuda.Stream()`` is -- that pass the premise of both scenarios.  Streams share the device's few hardware queues
        (four per process here), and two that share one run in order whatever the code does: such a pair shows nothing.  In a
        process that has used many streams before -- the whole suite -- a stream drawn from torch's pool shares the null
        stream's queue one time in four (measured: both directions waited the full 50 ms).  So streams are drawn ONE at a time,
        each tried against the null stream (and T against S) under 50 ms gates, until two will do: two drawn when the module
        runs alone, at most eight; the module fails, loudly, if those do not hold a pair.  Every stream has run something
        before its first gate: its first use sets up its queue."""
        torch = self.torch
        seen = []

        def passes(gated, other, what):
            ok, ms = self._passes(gated, other)
            seen.append(f"{what}: {'ok' if ok else 'BLOCKED'} ({ms:.1f} ms)")
            return ok

        S = T = None
        last = []
        for i in range(8):
            x = torch.cuda.Stream()
            last = (last + [x])[-2:]
            with torch.cuda.stream(x):
                self.tiny[1].copy_(self.tiny[0])
            torch.cuda.synchronize()
            if not (passes(x, self.NULL, f"gate on {i}, copy on null") and passes(self.NULL, x, f"gate on null, copy on {i}")):
                continue
            if S is None:
                S = x
            elif passes(S, x, f"gate on S, copy on {i}") and passes(x, S, f"gate on {i}, copy on S"):
                T = x
                break
        print("\nstream-order premise trials: " + "; ".join(seen))
        if T is not None:
            return S, T, {"A": True, "B": True}
        return last[0], last[-1], {"A": False, "B": False}

    def require_premise(self, scenario):
        assert self.gate_50_ms >= 0.8 * GATE_MIN_MS, f"a gate asked to last 50 ms lasted {self.gate_50_ms} ms"
        assert self.premise[scenario], \
            f"scenario {scenario}: a copy on another stream did not complete while the gate was pending -- the streams share a " \
            "hardware queue, so nothing here could tell a wrong stream from the right one"

    def require_case_premise(self, g, what):
        """The premise once more, for ONE gated call: established when the streams were picked, it holds for a case only if the
        streams were still served independently while that case's gate was pending -- and if the host was not held up for longer
        than the gate between queueing it and making the call.  Without it a match proves nothing and a mismatch neither."""
        assert g.premise, \
            f"{what}: the premise did not hold for this case -- the work on the ungated stream had not completed when the gate ran " \
            "out (the two streams were served one behind the other, or the host stalled for longer than the gate): the case shows " \
            "nothing about the library"

    def gate_length(self, kind, host_ms):
        """G = max(50 ms, 10 x the host time of the ungated call), at most 500 ms; both filed in the report under `kind`"""
        gate_ms = min(GATE_MAX_MS, max(GATE_MIN_MS, GATE_FACTOR * host_ms))
        r = self.report.setdefault(kind, [host_ms, host_ms, gate_ms, gate_ms, 0])
        r[0], r[1], r[2], r[3], r[4] = min(r[0], host_ms), max(r[1], host_ms), min(r[2], gate_ms), max(r[3], gate_ms), r[4] + 1
        return gate_ms

    # -- calls
    def poison(self, job):
        for ar in job.arenas:
            ar.flat.fill_(ar.poison)

    def ungated(self, job, plan):
        """The call on an idle, synchronised device (on S: a run may capture a graph, which needs a stream of its own).  Returns
        (what it returned, the arenas' bits afterwards, the host time of the call in ms)."""
        torch = self.torch
        self.poison(job)
        for view, staged in job.uploads:
            view.copy_(staged)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ret = job.call(plan, self.S)
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        return ret, [ar.flat.clone() for ar in job.arenas], host_ms

    def reference(self, key, job):
        """Once per configuration: the ungated result of a fresh plan (its first call: cold; that run also loads the kernels'
        code objects), the host time of the same call on the then warm plan, and the gate length that follows from it."""
        if key in self.refs:
            return self.refs[key]
        plan = job.make_plan()
        ret, expected, _ = self.ungated(job, plan)
        ret2, again, host_ms = self.ungated(job, plan)
        assert repr(ret) == repr(ret2), (key, ret, ret2)
        for ar, x, y in zip(job.arenas, expected, again):
            assert self.torch.equal(x, y), f"{key}: the ungated call is not deterministic"
            A.assert_guards_intact(dataclasses.replace(ar, flat=x), f"{key} (ungated)")
        gate_ms = self.gate_length(job.kind, host_ms)
        self.refs[key] = Ref(plan, ret, expected, host_ms, gate_ms, job)
        return self.refs[key]

    def gated(self, job, plan, scenario, gate_ms, control=False, after_call=None, premise=True):
        """One gated call.  `premise`: also establish this case's own premise (Gated.premise) -- A: before the call a tiny copy on
        T and one on the null stream complete, and in the control T has drained after the snapshot, while S's gate is still
        pending; B: S has drained after the snapshot while the null stream's gate is still pending.  "Still pending" is the
        stream's query() AND the clock: less than half the gate's length since it was queued (a wait that returns just as the
        gate runs out can still find query() false)."""
        torch = self.torch
        S, T, NULL = self.S, self.T, self.NULL
        gated = S if scenario == "A" else NULL
        upload_on, call_on = S, S
        if control:  # the call on another stream than the one that carries the gated uploads
            if scenario == "A":
                call_on = T
            else:
                upload_on = NULL
        self.poison(job)
        torch.cuda.synchronize()
        self.gate(gated, gate_ms)
        t_gate = time.perf_counter()

        def early():  # the gate is still pending, and less than half of it has passed since it was queued
            return (not gated.query()) and (time.perf_counter() - t_gate) * 1e3 < 0.5 * gate_ms

        with torch.cuda.stream(upload_on):
            for view, staged in job.uploads:
                view.copy_(staged, non_blocking=True)
        held = None
        if premise and scenario == "A" and not control:
            held = True
            for other in (T, NULL):
                with torch.cuda.stream(other):
                    self.tiny[1].copy_(self.tiny[0])
                    self.done.record()
                self.done.synchronize()  # (bounded: at the latest when the gate has run out)
                held = held and early()
        t0 = time.perf_counter()
        ret = job.call(plan, call_on)
        host_ms = (time.perf_counter() - t0) * 1e3
        busy_after = not gated.query()
        drained_after = S.query()
        if after_call is not None:
            after_call()
        with torch.cuda.stream(call_on):
            for snap, ar in zip(job.snaps, job.arenas):
                snap.copy_(ar.flat, non_blocking=True)
                ar.flat.fill_(ar.poison)
        if premise and (scenario == "B" or control):
            call_on.synchronize()  # (bounded likewise)
            held = early()
        torch.cuda.synchronize()
        clean = all(bool((ar.flat == ar.poison).all()) for ar in job.arenas)
        return Gated(ret, busy_after, drained_after, host_ms, clean, held)

    def compare(self, job, ref, what):
        for i, (ar, snap, exp) in enumerate(zip(job.arenas, job.snaps, ref.expected)):
            bad = snap != exp
            n = int(bad.sum())
            assert n == 0, f"{what}: arena {i}: {n} of {snap.numel()} elements differ from the ungated call's, first at element " \
                           f"{int(bad.nonzero()[0])}; {int((snap == ar.poison).sum() - (exp == ar.poison).sum())} more of them poison"
            A.assert_guards_intact(dataclasses.replace(ar, flat=snap), what)

    def check(self, key, job, scenario, mode):
        """One gated call of a fresh plan (mode: "cold" / "prepared") against the reference of `key`."""
        self.require_premise(scenario)
        ref = self.reference(key, job)
        plan = job.make_plan()
        if mode == "prepared":
            if job.prepare is not None:
                job.prepare(plan)
            else:
                self.ungated(job, plan)
            self.torch.cuda.synchronize()
        g = self.gated(job, plan, scenario, ref.gate_ms)
        what = f"{key} scenario {scenario} {mode} (gate {ref.gate_ms:.0f} ms, host {g.host_ms:.2f} ms, busy after: {g.busy_after})"
        print("stream-order:", what)
        self.require_case_premise(g, what)
        self.compare(job, ref, what)
        assert repr(g.ret) == repr(ref.ret), (what, g.ret, ref.ret)
        assert g.clean, f"{what}: something wrote into the grids after the caller's stream had put the poison back"
        if mode == "cold":
            return g
        if not job.blocking:
            assert g.busy_after, f"{what}: the call blocked until the gated stream had drained"
        elif scenario == "A":
            assert g.drained_after, f"{what}: a blocking entry returned before its stream had drained"
        else:
            assert g.busy_after, f"{what}: a blocking entry waited for the null stream, not for its own"
        return g


@pytest.fixture(scope="module")
def ctx(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L
    from oracle import oracle as O

    c = Ctx(L, O)
    yield c
    torch.cuda.synchronize()
    print("\nstream-order report: kind, host ms (min .. max), gate ms (min .. max), configurations")
    for kind, (h0, h1, g0, g1, n) in sorted(c.report.items()):
        print(f"stream-order report: {kind:28s} {h0:8.3f} .. {h1:8.3f}   {g0:6.1f} .. {g1:6.1f}   {n}")
    c.refs.clear()


def _bits(torch, a):
    """a host array (fp64, or bf16 as uint16) as a staged integer tensor on the device"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16 if a.dtype.itemsize == 2 else np.int64).copy()).cuda()


def _second_buffer(ctx, ar, shape, boundary):
    """Buffer 1 before a run, as poisoned as lora_plan_run's contract allows (test_gpu_memory_contract._fill_second): under the
    reference boundary its halo is zero and its interior poison; otherwise poison everywhere."""
    torch = ctx.torch
    s = torch.full(ar.padded_shape, ar.poison, dtype=ar.flat.dtype, device="cuda")
    if boundary in (None, "reference"):
        s.zero_()
        ctx.L.ops.interior(shape, s).fill_(ar.poison)
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# the premise and the negative controls
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_premise_a_copy_on_another_stream_completes_while_the_gate_is_pending(ctx, scenario):
    ctx.require_premise(scenario)


def _run_job(ctx, row, kind="run"):
    """lora_plan_run of a row of test_gpu_memory_contract.ROWS: the ragged size, the last of its step counts."""
    dims, t = row.ragged, row.times[-1]
    ar = A.carve(ctx.O.padded_shape(row.shape, dims), row.dtype, 2, A.OFFSETS[ROW_IDS.index(row.id) % 5])
    uploads = [(ar.bits(0), _bits(ctx.torch, _input(ctx.O, row, dims))), (ar.bits(1), _second_buffer(ctx, ar, row.shape, row.bc))]
    return Job(kind, [ar], uploads, lambda: _make_plan(ctx.L, ctx.O, row, dims),
               lambda plan, s: plan.run(ar.views[0], ar.views[1], t, stream=s), prepare=lambda plan: plan.prepare_run(t))


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_negative_control_a_call_on_the_wrong_stream_does_not_match(ctx, scenario):
    """The method can fail: the same run handed another stream than the one that carries the gated uploads (A: the call on a
    second stream while S is gated; B: the uploads behind the null stream's gate) reads the poison -- allocated memory, nothing
    faults -- and its snapshot is not the ungated call's."""
    ctx.require_premise(scenario)
    row = ROWS[ROW_IDS.index("2d_wg6")]
    ref = _run_ref(ctx, row)
    job = ref.job
    plan = job.make_plan()
    plan.prepare_run(row.times[-1])
    ctx.torch.cuda.synchronize()
    g = ctx.gated(job, plan, scenario, ref.gate_ms, control=True)
    ar, snap, exp = job.arenas[0], job.snaps[0], ref.expected[0]
    same = ctx.torch.equal(snap, exp)
    print(f"stream-order: control {scenario}: premise held: {g.premise}, busy after: {g.busy_after}, host {g.host_ms:.2f} ms, "
          f"matched: {same}, poison in the result: {int((snap[ar.spans[row.times[-1] % 2][0]:ar.spans[row.times[-1] % 2][1]] == ar.poison).sum())}")
    ctx.require_case_premise(g, f"control, scenario {scenario}")  # (before the bits are judged: they mean nothing without it)
    assert not same, f"scenario {scenario}: the call on the wrong stream matched: the gate shows nothing"
    lo, hi = ar.spans[row.times[-1] % 2]
    assert bool((snap[lo:hi] == ar.poison).any()), "the wrong-stream result holds no poison"
    # ... and the same plan and buffers, the call on the right stream again: the bits of the ungated call
    g = ctx.gated(job, plan, scenario, ref.gate_ms)
    ctx.require_case_premise(g, f"after the control, scenario {scenario}")
    ctx.compare(job, ref, f"after the control, scenario {scenario}")


# ---------------------------------------------------------------------------------------------------------------------------
# 1. lora_plan_run over every kernel
# ---------------------------------------------------------------------------------------------------------------------------
# The rows whose last step count goes through the plan's scratch grid (capi.cpp: run_schedule -- an odd number, >= 3, of fused
# launches); each case asserts from lora_plan_run_profiled's launch counts that its row is filed rightly.
SCRATCH_ROWS = {
    "1d_fused2", "1d_fused4", "1d_fused8", "1d_fused16", "1d_fused32", "2d_tile", "2d_tile_persistent", "2d_stream4_even",
    "2d_stream4_odd", "2d_stream2_even", "2d_stream2_odd", "2d_wg4", "2d_wg2", "2d_wg6_49_taps", "3d_tile", "3d_planes_k2_w4",
    "3d_planes_k2_w8", "3d_planes_27_tap_order", "3d_lanes", "3d_lanes_spans0", "3d_lanes_spans1", "3d_lanes_spans2",
    "3d_lanes_z_chunk", "3d_lanes_odd", "bf16_fused2", "bf16_fused2_star", "bf16_lanes",
}
TORUS_ROWS = {"periodic_torus_1d", "periodic_torus_2d", "periodic_torus_3d"}
assert SCRATCH_ROWS | TORUS_ROWS <= set(ROW_IDS)
RUN_CASES = [(r, sc, mode) for r in ROWS for sc in SCENARIOS
             for mode in (("prepared", "cold") if r.id in SCRATCH_ROWS | TORUS_ROWS else ("prepared",))]


def _run_ref(ctx, row):
    """The reference of a row's run, made once; the row is filed rightly: the scratch grid exactly where SCRATCH_ROWS says, fused
    launches on the torus rows."""
    key = ("run", row.id)
    if key in ctx.refs:
        return ctx.refs[key]
    ref = ctx.reference(key, _run_job(ctx, row))
    ar = ref.job.arenas[0]
    prof = ref.plan.run_profiled(ar.views[0], ar.views[1], row.times[-1])
    ctx.torch.cuda.synchronize()
    n = prof.fused_launches + prof.two_launches
    natural = row.ndim == 3 and ref.plan.get_option("steps_per_launch") == 3
    scratch = row.bc != "periodic" and not natural and n >= 3 and n % 2 == 1 and row.opts.get("scratch", -1) != 0
    assert scratch == (row.id in SCRATCH_ROWS), (row.id, prof.fused_launches, prof.two_launches, prof.single_launches)
    if row.id in TORUS_ROWS:
        assert n > 0, row.id
    return ref


@pytest.mark.parametrize("row,scenario,mode", RUN_CASES, ids=[f"{r.id}-{sc}-{m}" for r, sc, m in RUN_CASES])
def test_run_is_ordered_on_its_stream(ctx, row, scenario, mode):
    ctx.check(("run", row.id), _run_ref(ctx, row).job, scenario, mode)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. every branch of the run skeleton (capi.cpp: run_launches, run_torus, lora_plan_run's graph), at small shapes
# ---------------------------------------------------------------------------------------------------------------------------
# id: shape, dims, boundary, options, sweeps, the launches lora_plan_run_profiled must report (fused, shallower, single)
BRANCHES = {
    "reference_even": ("star2d1r", (40, 130), None, {"steps_per_launch": 2}, 4, (2, 0, 0)),
    "reference_odd_scratch": ("star2d1r", (40, 130), None, {"steps_per_launch": 2}, 7, (3, 0, 1)),
    "natural_3d": ("box3d1r", (9, 31, 62), None, {"steps_per_launch": 3, "stream3_waves": 8}, 10, (2, 2, 0)),
    "dirichlet_2d": ("star2d1r", (53, 246), "dirichlet", {}, 13, (3, 0, 1)),
    "dirichlet_3d": ("star3d1r", (9, 20, 136), "dirichlet", {}, 7, (3, 0, 1)),
    "periodic_sweeps": ("box2d3r", (40, 130), "periodic", {"torus": 0}, 7, (0, 0, 7)),
    "torus": ("star2d1r", (53, 246), "periodic", {}, 7, None),
}
BRANCH_CASES = [(b, sc, m) for b in BRANCHES for sc in SCENARIOS for m in ("prepared", "cold")]


def _plain_plan(ctx, shape, dims, bc, opts, graph=None):
    w = ctx.O.effective_weights(shape)
    plan = ctx.L.Plan(shape, dims).set_weights(w / w.sum())
    if bc:
        plan.set_boundary(bc)
    for k, v in opts.items():
        plan.set_option(k, v)
    if graph is not None:
        plan.set_option("graph", graph)
    return plan


def _plain_run_job(ctx, kind, shape, dims, bc, opts, t, offset, graph=None):
    ps = ctx.O.padded_shape(shape, dims)
    ar = A.carve(ps, "f64", 2, offset)
    a = np.random.default_rng(len(kind) + t).standard_normal(ps)
    uploads = [(ar.bits(0), _bits(ctx.torch, a)), (ar.bits(1), _second_buffer(ctx, ar, shape, bc))]
    return Job(kind, [ar], uploads, lambda: _plain_plan(ctx, shape, dims, bc, opts, graph),
               lambda plan, s: plan.run(ar.views[0], ar.views[1], t, stream=s), prepare=lambda plan: plan.prepare_run(t))


@pytest.mark.parametrize("branch,scenario,mode", BRANCH_CASES, ids=[f"{b}-{sc}-{m}" for b, sc, m in BRANCH_CASES])
def test_run_skeleton_branches_are_ordered_on_their_stream(ctx, branch, scenario, mode):
    shape, dims, bc, opts, t, launches = BRANCHES[branch]
    key = ("branch", branch)
    if key not in ctx.refs:
        ref = ctx.reference(key, _plain_run_job(ctx, "run (skeleton branch)", shape, dims, bc, opts, t, 48))
        ar = ref.job.arenas[0]
        prof = ref.plan.run_profiled(ar.views[0], ar.views[1], t)
        ctx.torch.cuda.synchronize()
        got = (prof.fused_launches, prof.two_launches, prof.single_launches)
        assert got == launches if launches else got[0] + got[1] > 0, (branch, got)  # the branch is the one its name says
    ctx.check(key, ctx.refs[key].job, scenario, mode)


def test_a_cold_run_still_in_flight_when_the_null_streams_gate_runs_out(ctx):
    """Scenario B on a run that OUTLASTS the gate.  Whatever a cold call leaves on the null stream starts when the gate runs out;
    in every other case the run on S has long finished by then, so such work can only be seen if it lands in the caller's grids.
    Here the run is still in flight: 3001 launches of six sweeps on a 2048 x 2048 grid -- an odd number, so the last two hops go
    through the scratch grid, whose ring was copied from buffer 0 at the very start of the run -- take well over the 50 ms of the
    gate (the case asserts that they did).  A scratch grid zeroed on the null stream during first-need allocation loses that ring
    in mid-run and the last launch reads zeros for it: with the hipMemset that DeviceGrid::ensure used to issue, 146160 cells of
    the result differed ("Stream ordering").  Measured: a launch takes about 60 us as enqueued here (9001 of them 555
    ms), so the run lasts some 185 ms.  The gate is the shortest one whatever the host time of the call: the question is what
    starts when it runs out, and being cold the case asserts the result alone."""
    ctx.require_premise("B")
    torch = ctx.torch
    shape, dims, launches = "star2d1r", (2048, 2048), 3001
    key = ("long", shape)
    job = _plain_run_job(ctx, "run (outlasts the gate)", shape, dims, None, {"graph": 0}, 6 * launches, 16)
    ref = ctx.reference(key, job)
    ar = job.arenas[0]
    prof = ref.plan.run_profiled(ar.views[0], ar.views[1], 6 * launches)
    torch.cuda.synchronize()
    assert (prof.fused_launches, prof.two_launches, prof.single_launches) == (launches, 0, 0)
    seen = {}

    def after_call():
        ctx.NULL.synchronize()  # (the gate: bounded)
        seen["in flight"] = not ctx.S.query()

    plan = job.make_plan()
    g = ctx.gated(job, plan, "B", GATE_MIN_MS, after_call=after_call, premise=False)  # (S outlasts the gate: its own condition)
    what = f"a run of {launches} launches, cold, scenario B (host {g.host_ms:.1f} ms, in flight when the gate ran out: {seen})"
    print("stream-order:", what)
    assert seen["in flight"], f"{what}: the run had finished before the gate ran out, so the case shows nothing"
    ctx.compare(job, ref, what)
    assert g.clean, what
    ctx.refs.pop(key)


GRAPHS = [("1d1r", (1 << 16,), 40), ("star2d1r", (128, 256), 21)]  # test_graph_replay_of_launch_bound_runs


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("shape,dims,t", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_graph_captured_runs_are_ordered_on_their_stream(ctx, shape, dims, t, scenario):
    """graph = 1: the first gated call captures, instantiates and launches the graph (the result alone is asserted: set-up); the
    second one, under a gate of its own, replays the cached graph and must not block either."""
    ctx.require_premise(scenario)
    key = ("graph", shape, scenario)  # (its own buffers and reference per scenario: the cases stay independent)
    job = _plain_run_job(ctx, "run (graph)", shape, dims, None, {}, t, 112, graph=1)
    try:
        ref = ctx.reference(key, job)
        plan = job.make_plan()
        plan.prepare_run(t)
        ctx.torch.cuda.synchronize()
        for step in ("capture", "replay"):
            g = ctx.gated(job, plan, scenario, ref.gate_ms)
            what = f"graph {shape} scenario {scenario} {step} (host {g.host_ms:.2f} ms, busy after: {g.busy_after})"
            print("stream-order:", what)
            ctx.require_case_premise(g, what)
            ctx.compare(job, ref, what)
            assert g.clean, what
            if step == "replay":
                assert g.busy_after, f"{what}: the replay blocked until the gated stream had drained"
    finally:
        ctx.torch.cuda.synchronize()
        ctx.refs.pop(key, None)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the raw launch entries on S, under scenario A: one row per kernel family (the launchers all take the stream)
# ---------------------------------------------------------------------------------------------------------------------------
FAMILY_ROWS = ["1d_single", "1d_fused8", "2d_direct", "2d_generic", "2d_mfma", "2d_tile", "2d_stream4_even", "2d_wg6",
               "2d_wg4_dirichlet", "3d_single", "3d_generic", "3d_tile", "3d_planes_k3_w4", "3d_lanes", "bf16_single_lds_dma",
               "bf16_fused2", "bf16_lanes", "bf16_mfma"]


@pytest.mark.parametrize("row_id", FAMILY_ROWS)
def test_raw_launch_entries_are_ordered_on_their_stream(ctx, row_id):
    """step, step_region, step2, stepk and stepn_region2 of one plan, each into a destination of its own, behind ONE gate on S;
    every destination starts as poison (its halo stays poison: these are raw sweeps)."""
    row = ROWS[ROW_IDS.index(row_id)]
    dims = row.ragged
    n = dims[0]
    probe = _make_plan(ctx.L, ctx.O, row, dims)
    g = probe.region_granularity
    K = probe.get_option("steps_per_launch") if row.fused_direct else 1
    lo, hi = max(g, (n // 4) // g * g), max(n // 2, (n - n // 4)) // g * g   # (test_gpu_memory_contract: two ranges in one call)
    rb, re = min(n, n // 3 + 1) // g * g, min(n, 2 * n // 3 + 2)
    entries = [lambda p, s, d, st: p.step(s, d, stream=st), lambda p, s, d, st: p.step_region(s, d, rb, re, stream=st)]
    if row.step2:
        entries.append(lambda p, s, d, st: p.step2(s, d, stream=st))
    if row.fused_direct:
        entries.append(lambda p, s, d, st: p.stepk(s, d, stream=st))
    entries.append(lambda p, s, d, st: p.stepn_region2(K, s, d, 0, lo, hi, n, stream=st))
    ar = A.carve(ctx.O.padded_shape(row.shape, dims), row.dtype, 1 + len(entries), A.OFFSETS[ROW_IDS.index(row.id) % 5])

    def call(plan, st):
        for i, e in enumerate(entries):
            e(plan, ar.views[0], ar.views[1 + i], st)

    job = Job("raw launches (4 - 5 calls)", [ar], [(ar.bits(0), _bits(ctx.torch, _input(ctx.O, row, dims)))],
              lambda: _make_plan(ctx.L, ctx.O, row, dims), call, prepare=lambda plan: None)
    ctx.check(("raw", row.id), job, "A", "prepared")
    exp = ctx.refs.pop(("raw", row.id)).expected[0]
    for i in range(len(entries)):  # (every entry wrote something: the comparison above was not poison against poison)
        b, e = ar.spans[1 + i]
        assert bool((exp[b:e] != ar.poison).any()), (row.id, i)


@pytest.mark.parametrize("shape,dims,dtype", [("1d1r", (37,), "f64"), ("box2d3r", (40, 131), "f64"), ("box3d1r", (9, 31, 248), "bf16")])
def test_halo_and_block_copy_entries_are_ordered_on_their_stream(ctx, shape, dims, dtype):
    """lora_plan_halo in its three modes and (fp64) lora_copy_block_f64, each into a buffer of its own, behind one gate on S."""
    from lorastencil_amd import _lib
    from lorastencil_amd.ops import _stream

    torch, O = ctx.torch, ctx.O
    ps = O.padded_shape(shape, dims)
    rng = np.random.default_rng(3)
    enc = O.to_bf16 if dtype == "bf16" else (lambda x: x)
    ar = A.carve(ps, dtype, 5, 48)
    uploads = [(ar.bits(i), _bits(torch, enc(rng.integers(1, 90, ps).astype(np.float64)))) for i in range(4)]
    # a block inside the grid seen as rows of its innermost extent (a 1D array: one row)
    ld, total = ps[-1], int(np.prod(ps[:-1]))
    r0 = 1 if total > 2 else 0
    rows, cols = total - 2 * r0, ld - 3

    def call(plan, st):
        plan.halo(ar.views[1], "copy", ar.views[0], stream=st)
        plan.halo(ar.views[2], "zero", stream=st)
        plan.halo(ar.views[3], "wrap", stream=st)
        if dtype == "f64":
            _lib.check(_lib.lib().lora_copy_block_f64(ar.views[4].data_ptr() + (r0 * ld + 1) * 8, ld, ar.views[0].data_ptr() + (r0 * ld + 2) * 8,
                                                      ld, rows, cols, _stream(st)), "lora_copy_block_f64")

    job = Job("halo x 3, block copy", [ar], uploads, lambda: ctx.L.Plan(shape, dims, dtype=dtype), call, prepare=lambda plan: None)
    ctx.check(("halo", shape, dtype), job, "A", "prepared")
    exp = ctx.refs.pop(("halo", shape, dtype)).expected[0]
    b, e = ar.spans[4]
    assert bool((exp[b:e] != ar.poison).any()) == (dtype == "f64")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. drivers with plan-owned grids, and the blocking entries
# ---------------------------------------------------------------------------------------------------------------------------
DRIVER_CONFIGS = [(s, d, leap3) for s, d, _ in RUNS if len(d) >= 2 for leap3 in ((0, 1) if len(d) == 3 else (0,))]
DRIVER_KINDS = ("run_leapfrog", "run_leapfrog_src", "run_with_source", "chebyshev_until_max", "chebyshev_until_rms")
UNTIL_KINDS = ("run_until_max", "run_until_rms")
REDUCTIONS = ("stats", "diff", "residual", "residual_src")
DRIVER_CASES = [(s, d, l3, k) for s, d, l3 in DRIVER_CONFIGS for k in DRIVER_KINDS] + \
               [(s, d, l3, k) for s, d, l3 in DRIVER_CONFIGS if len(d) == 2 for k in UNTIL_KINDS] + \
               [(s, d, 0, k) for s, d in (("star2d1r", (70, 260)), ("box3d1r", (35, 17, 130))) for k in REDUCTIONS]
assert all((s, d, 0) in DRIVER_CONFIGS for s, d, _, k in DRIVER_CASES if k in REDUCTIONS)


def _driver_job(ctx, shape, dims, leap3, kind):
    """prev, cur, f carved out of one poisoned allocation, their seeded inputs (test_gpu_leapfrog_src.host_data: the halos differ
    too) uploaded behind the gate."""
    L, torch = ctx.L, ctx.torch
    ar = A.carve(L.padded_shape(shape, dims), "f64", 3, 240)
    prev, cur, f = ar.views
    h_prev, h_cur, h_f = host_data(shape, dims)
    w = real_taps(L, shape)
    a, c = L.chebyshev_coeffs(RHO, 1, 8)
    bc = "dirichlet" if kind in UNTIL_KINDS else None
    second = h_prev
    if kind in ("run_with_source",) + UNTIL_KINDS:  # prev is buffer 1 of a plain run: as poisoned as the contract allows
        second = None

    def make_plan():
        plan = L.Plan(shape, dims).set_weights(w)
        if bc:
            plan.set_boundary(bc)
        if leap3:
            plan.set_option("leap3", 1)
        if kind == "run_with_source":
            plan.set_source(f)
        return plan

    calls = {
        "run_leapfrog": lambda p, s: p.run_leapfrog(prev, cur, -0.9, 9, stream=s),  # two pairs of two-step launches and a tail
        "run_leapfrog_src": lambda p, s: p.run_leapfrog_src(prev, cur, f, a, c, 8, stream=s),
        "run_with_source": lambda p, s: p.run(cur, prev, 7, stream=s),  # 2D: 2 + 2 + 2 through the scratch grid, + 1
        "chebyshev_until_max": lambda p, s: p.run_chebyshev_until(prev, cur, f, RHO, norm="max", stream=s, **UNTIL),
        "chebyshev_until_rms": lambda p, s: p.run_chebyshev_until(prev, cur, f, RHO, norm="rms", stream=s, **UNTIL),
        "run_until_max": lambda p, s: p.run_until(cur, prev, norm="max", stream=s, **UNTIL),
        "run_until_rms": lambda p, s: p.run_until(cur, prev, norm="rms", stream=s, **UNTIL),
        "stats": lambda p, s: p.stats(cur, stream=s),
        "diff": lambda p, s: p.diff(cur, prev, stream=s),
        "residual": lambda p, s: p.residual(cur, stream=s),
        "residual_src": lambda p, s: p.residual_src(cur, f, stream=s),
    }
    uploads = [(ar.bits(0), _bits(torch, h_prev) if second is not None else _second_buffer(ctx, ar, shape, bc)),
               (ar.bits(1), _bits(torch, h_cur)), (ar.bits(2), _bits(torch, h_f))]
    return Job(kind, [ar], uploads, make_plan, calls[kind], blocking="until" in kind or kind in REDUCTIONS)


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("shape,dims,leap3,kind", DRIVER_CASES,
                         ids=[f"{s}-{'x'.join(map(str, d))}-leap3={l3}-{k}" for s, d, l3, k in DRIVER_CASES])
def test_drivers_with_plan_owned_grids_are_ordered_on_their_stream(ctx, shape, dims, leap3, kind, scenario):
    """Cold (the leapfrog grids, the scratch grid, the probe grid, the records are allocated inside the gated call), then prepared
    (a plan that has made the same call once).  The until-drivers' and the reductions' records equal the ungated ones."""
    key = ("driver", shape, dims, leap3, kind)
    if key not in ctx.refs:
        ref = ctx.reference(key, _driver_job(ctx, shape, dims, leap3, kind))
        if "until" in kind:
            assert ref.ret.times_done == UNTIL["max_times"] and ref.ret.checks == 2, ref.ret  # (both probes ran)
        if kind in REDUCTIONS:
            assert ref.ret.count == int(np.prod(dims)), ref.ret
    job = ctx.refs[key].job
    ctx.check(key, job, scenario, "cold")
    ctx.check(key, job, scenario, "prepared")
    if scenario == SCENARIOS[-1]:
        ctx.refs.pop(key)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the C++ slab and block drivers over loopback: the gate on every slab's / block's own sweep stream
# ---------------------------------------------------------------------------------------------------------------------------
def _gated_decomposition(ctx, kind, make, n, a, times, check_oracle, what):
    """`make()` builds the slabs / blocks; one set runs ungated (and is timed), a second one with a gate on each member's sweep
    stream between load and run: an exchange on a communication stream that is served while the gates are pending runs ahead of
    the strips it must wait for unless its event wait is in place.  The streams share the device's few hardware queues, and a
    communication stream that shares one with a gated sweep stream is held back by that gate whatever the code does; so the case
    has a premise of its own -- with every sweep stream gated, a tiny copy completes on at least one communication stream -- and
    prints how many of them were free.  Bit for bit the ungated result, and the oracle as the existing loopback test demands it."""
    torch = ctx.torch
    plain = make()
    plain.load(a)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plain.run(times // 2)  # (resumed, as in the existing tests)
    plain.run(times - times // 2)
    host_ms = (time.perf_counter() - t0) * 1e3
    plain.sync()
    want = plain.store(np.zeros_like(a))
    gate_ms = ctx.gate_length(kind, host_ms)

    gated = make()
    streams = [torch.cuda.ExternalStream(gated.stream(i)) for i in range(n)]
    assert n >= 2 and all(s.cuda_stream for s in streams)
    gated.load(a)
    torch.cuda.synchronize()
    comm = [torch.cuda.ExternalStream(gated.comm_stream(i)) for i in range(n)]
    assert all(c.cuda_stream for c in comm)
    for c in comm:  # (a stream's first use sets up its queue: not behind a gate)
        with torch.cuda.stream(c):
            ctx.tiny[1].copy_(ctx.tiny[0])
    torch.cuda.synchronize()
    for s in streams:
        ctx.gate(s, gate_ms)
    free, t_gate = 0, time.perf_counter()
    for c in comm:
        with torch.cuda.stream(c):
            ctx.tiny[1].copy_(ctx.tiny[0])
            ctx.done.record()
        ctx.done.synchronize()  # (bounded: at the latest when the gates have run out)
        free += (not any(s.query() for s in streams)) and (time.perf_counter() - t_gate) * 1e3 < 0.5 * gate_ms
    torch.cuda.synchronize()  # (a wait on a stream that was held back has used the gates up: the run gets fresh ones)
    for s in streams:
        ctx.gate(s, gate_ms)
    gated.run(times // 2)
    gated.run(times - times // 2)
    busy = not all(s.query() for s in streams)
    gated.sync()
    got = gated.store(np.zeros_like(a))
    torch.cuda.synchronize()
    print(f"stream-order: {what} (gate {gate_ms:.0f} ms on {n} streams, host {host_ms:.2f} ms, busy after: {busy}, "
          f"communication streams served while every sweep stream was gated: {free} of {n})")
    assert free >= 1, f"{what}: no communication stream was served while the sweep streams were gated: the case shows nothing"
    assert busy, f"{what}: run() blocked until the gated sweep streams had drained"
    differ = got.view(np.int64) != want.view(np.int64)
    assert not differ.any(), f"{what}: {int(differ.sum())} cells differ from the ungated run"
    check_oracle(got)
    plain.close()
    gated.close()


SLABS = [("star2d1r", (768, 384), 2, 23, 2, {"steps_per_launch": 4}), ("star3d1r", (24, 20, 64), 3, 7, 2, None)]
BLOCKS = [("star2d1r", (768, 1024), (2, 2), 16, 2, None), ("star3d1r", (48, 40, 128), (2, 2), 9, 2, None)]


@pytest.mark.parametrize("flags", [0, 16], ids=["default", "overlap"])
@pytest.mark.parametrize("shape,dims,nranks,times,every,opts", SLABS, ids=[s[0] for s in SLABS])
def test_slab_driver_exchanges_wait_for_the_gated_sweep_streams(ctx, shape, dims, nranks, times, every, opts, flags):
    """rows of test_cslab.test_loopback_slabs_equal_single_gpu, with the default flags and with SLAB_OVERLAP (boundary strips first)"""
    from lorastencil_amd import cslab

    assert cslab.SLAB_OVERLAP == 16
    a = ctx.O.reference_input(shape, dims)
    what = f"slab driver: {shape} {dims} x {nranks} flags {flags}"

    def check_oracle(got):
        exp = ctx.O.run(shape, a, times)
        if np.abs(exp).max() < 2.0 ** 50:
            assert np.array_equal(got, exp), what
        else:
            assert np.abs(got - exp).max() <= 1e-13 * np.abs(exp).max(), what

    _gated_decomposition(ctx, "slab driver (run)", lambda: cslab.SlabSet(shape, dims, nranks, comms=cslab.loopback_comms(nranks),
                                                                         exchange_every=every, flags=flags, options=opts),
                         nranks, a, times, check_oracle, what)


@pytest.mark.parametrize("flags", [0, 16], ids=["default", "overlap"])
@pytest.mark.parametrize("shape,dims,grid,times,every,opts", BLOCKS, ids=[b[0] for b in BLOCKS])
def test_block_driver_exchanges_wait_for_the_gated_sweep_streams(ctx, shape, dims, grid, times, every, opts, flags):
    """rows of test_cblocks.test_loopback_blocks_equal_the_undivided_grid (normalised taps on real data, as there)"""
    from lorastencil_amd import cblocks

    O = ctx.O
    w = O.effective_weights(shape)
    w = w / w.sum()
    a = np.random.default_rng(2).standard_normal(O.padded_shape(shape, dims))
    n = grid[0] * grid[1]
    what = f"block driver: {shape} {dims} {grid[0]} x {grid[1]} flags {flags}"

    def check_oracle(got):
        exp = O.run(shape, a, times, weights=w)
        assert np.abs(got - exp).max() <= 1e-13 * np.abs(exp).max(), what

    _gated_decomposition(ctx, "block driver (run)", lambda: cblocks.BlockGrid(shape, dims, grid, comms=cblocks.loopback_comms(n), weights=w,
                                                                            exchange_every=every, flags=flags, options=opts),
                         n, a, times, check_oracle, what)
