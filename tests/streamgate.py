"""Stream-order harness: does every launch of a call ride the caller's stream?

Every device entry point promises stream order on the stream it is handed (or
on torch's current stream).  A test that passes the null stream on an idle
device cannot tell: whatever stream a launch went to, it has finished by the
time torch reads the result back.  Here the call runs on a side stream ``S``
while a gate (``torch.cuda._sleep``, a one-thread spin kernel that leaves the
CUs free) is still running, so a launch on any other stream is caught.  The
one fact all of this rests on: torch's side streams are non-blocking, so the
null stream and a ``torch.cuda.Stream()`` do not wait for each other — which
``power_check`` verifies at run time with a deliberately mis-streamed call.

Arrangement A, gate ahead.  Queued on ``S`` with no host synchronisation in
between: the gate; an event ``g_end``; device-to-device copies of the real
inputs into the buffers the call reads (until then they hold POISON1); the
call; copies of every output into pinned host memory; POISON2 over the
inputs.  A launch the call placed on another stream runs while the inputs are
still poison (or, if late, already poison again).

Arrangement B, gate elsewhere.  The gate is queued on the NULL stream; on the
idle ``S``: the call, the copy-out, POISON2 over the inputs.  ``S`` is
synchronised first, then the device.  A launch that went to the null stream
has not run when the outputs are read: the sentinel shows.

Condition, not measurement: in A ``g_end.query()`` must be False right after
the call returns, in B the null-stream gate's end event must be False after
the copy-out is queued.  A case where it is not FAILS ("gate too short / call
blocked the host"); it is never skipped or counted as passed.

Gate length.  ``_sleep`` is timed once per process with events and scaled to
GATE_MS.  Measured on one MI355X machine (one run of both stream-order
modules): gate 60.0 ms; slowest host issue time of any case 3.2 ms (the
two-model drop-in's first call; 1.3 ms in the C ABI module), taken with
time.perf_counter around the queueing of arrangement A, gate to second
poison.  The gate is more than 4x that (18x), and under the 200 ms cap.  The
figures are from one machine; the condition above, not they, is what each
case checks.
"""
import functools
import gc
import time
from types import SimpleNamespace

import numpy as np
import torch

GATE_MS = 60.0            # target gate length; see the docstring for the measurement
GATE_CAP_MS = 200.0
_CAL_CYCLES = 20_000_000

F32_P1, F32_P2 = 12345.0, 54321.0
I64_P1, I64_P2 = 12345, 54321
H16_P1, H16_P2 = 123.0, 321.0      # exact in fp16 and in bf16

ISSUE = {"slowest_ms": 0.0, "case": None, "gate_ms": None}


def _bits32(v):
    return int(np.array([v], np.float32).view(np.int32)[0])


def _bits16(v, dtype):
    return int(torch.tensor([v], dtype=dtype).view(torch.int16)[0])


def poisons(kind):
    """(POISON1, POISON2) as fill values for a tensor of ``kind``: "f32",
    "i64", "f16", "bf16", or the raw-bit views the kernel tests keep their
    buckets in — "f32bits" (int32), "f16bits" / "bf16bits" (int16)."""
    if kind == "f32":
        return F32_P1, F32_P2
    if kind == "i64":
        return I64_P1, I64_P2
    if kind in ("f16", "bf16"):
        return H16_P1, H16_P2
    if kind == "f32bits":
        return _bits32(F32_P1), _bits32(F32_P2)
    dt = {"f16bits": torch.float16, "bf16bits": torch.bfloat16}[kind]
    return _bits16(H16_P1, dt), _bits16(H16_P2, dt)


KIND_OF = {torch.float32: "f32", torch.int64: "i64", torch.float16: "f16",
           torch.bfloat16: "bf16", torch.int32: "f32bits"}


class In:
    """A device buffer the call reads (whole tensor, guard bands included).
    ``real`` is staged on the device from the tensor's current contents.
    ``get``: where the call may re-home the data (a module's parameter moved
    into an arena by its first round), the way to the tensor that holds it now."""

    def __init__(self, t, kind=None, get=None):
        self._t, self.get = t, get
        self.real = t.detach().clone()
        self.p1, self.p2 = poisons(kind or KIND_OF[t.dtype])

    @property
    def t(self):
        return (self._t if self.get is None else self.get()).detach()

    def restage(self):
        """Take the tensor's current contents as the real input (a new round)."""
        self.real.copy_(self.t)


@functools.lru_cache(maxsize=None)
def gate_cycles():
    """_sleep cycles for GATE_MS, from one timed _sleep on this device."""
    torch.cuda.synchronize()
    torch.cuda._sleep(1000)                       # load the kernel
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(_CAL_CYCLES)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b)
    assert ms > 0.5, ("_sleep calibration", ms)
    target = min(GATE_MS, GATE_CAP_MS)
    cycles = int(_CAL_CYCLES * target / ms)
    # measure the gate as it will run
    a.record()
    torch.cuda._sleep(cycles)
    b.record()
    torch.cuda.synchronize()
    ISSUE["gate_ms"] = a.elapsed_time(b)
    assert ISSUE["gate_ms"] <= GATE_CAP_MS * 1.05, ISSUE
    return cycles


def _pinned_like(t):
    return torch.empty(t.shape, dtype=t.dtype, pin_memory=True)


def _np(t):
    """Host tensor -> numpy copy (bfloat16, which numpy lacks, as its int16 bits)."""
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return t.numpy().copy()


def run(arr, S, call, inputs, outputs, name, call_stream=None, out_like=None):
    """One case in arrangement ``arr`` ("A" / "B") on side stream ``S``.
    ``call(st)`` issues the call under test for torch stream ``st`` (it runs
    under ``torch.cuda.stream(st)``); ``call_stream`` overrides the stream it
    is handed (the power check's deliberate mis-stream) while the harness goes
    on believing ``S``.  ``inputs``: In objects; ``outputs``: device tensors,
    holding their sentinel — or a callable returning them once the call has
    been issued (tensors the call creates), with ``out_like`` tensors of their
    shapes and dtypes for the pinned copies.  Returns the outputs as they were
    right after the call on ``S`` (numpy, in order) and the inputs as they are
    at the end."""
    assert arr in ("A", "B")
    st = S if call_stream is None else call_stream
    null = torch.cuda.default_stream()
    assert S.cuda_stream != 0 and null.cuda_stream == 0
    cycles = gate_cycles()
    hosts = [_pinned_like(t) for t in (outputs if out_like is None else out_like)]
    g_end = torch.cuda.Event()
    for i in inputs:                              # set-up, on the null stream, then idle
        if arr == "A":
            i.t.fill_(i.p1)
        else:
            i.t.copy_(i.real)
    # no collection inside the bracket: a dead module's buckets going back to
    # the runtime there would block the host on the device, whatever the call does
    gc.collect()
    torch.cuda.synchronize()
    gc.disable()
    try:
        return _bracket(arr, S, st, null, cycles, g_end, hosts, call, inputs, outputs, name,
                        call_stream)
    finally:
        gc.enable()


def _bracket(arr, S, st, null, cycles, g_end, hosts, call, inputs, outputs, name, call_stream):
    t0 = time.perf_counter()
    with torch.cuda.stream(S if arr == "A" else null):
        torch.cuda._sleep(cycles)
        g_end.record()
    with torch.cuda.stream(S):
        if arr == "A":
            for i in inputs:
                i.t.copy_(i.real, non_blocking=True)
    with torch.cuda.stream(st):
        call(st)
    if arr == "A":
        running = not g_end.query()
    with torch.cuda.stream(S):
        outs = outputs() if callable(outputs) else outputs
        assert len(outs) == len(hosts), (name, "outputs", len(outs), len(hosts))
        for h, t in zip(hosts, outs):
            assert h.shape == t.shape and h.dtype == t.dtype, (name, h.shape, t.shape, t.dtype)
            h.copy_(t.detach(), non_blocking=True)
        if arr == "B":
            running = not g_end.query()
        for i in inputs:
            i.t.fill_(i.p2)
    ms = (time.perf_counter() - t0) * 1e3
    S.synchronize()
    got = [_np(h) for h in hosts]
    torch.cuda.synchronize()
    if call_stream is None and arr == "A" and ms > ISSUE["slowest_ms"]:
        ISSUE["slowest_ms"], ISSUE["case"] = ms, name
    assert running, (name, arr, "gate too short / call blocked the host",
                     f"issue {ms:.2f} ms, gate {ISSUE['gate_ms']:.1f} ms")
    after = [_np(i.t.cpu()) for i in inputs]
    return SimpleNamespace(out=got, after=after, issue_ms=ms)


def assert_poison2(res, inputs, name, skip=()):
    """Arrangement A: every input buffer ends as POISON2 — nothing of the call
    ran after its place in the stream."""
    for k, (i, a) in enumerate(zip(inputs, res.after)):
        if k in skip:
            continue
        want = _np(torch.empty(1, dtype=i.t.dtype).fill_(i.p2))[0]
        assert (a == want).all(), \
            (name, "input", k, "written after the call's place in the stream")


def report():
    """The measured figures of this process, for the log."""
    return (f"streamgate: gate {ISSUE['gate_ms']} ms, slowest host issue "
            f"{ISSUE['slowest_ms']:.3f} ms ({ISSUE['case']})")


# ------------------------------------------------------------ power check ----
def power_check(arr, S):
    """The same call through the harness with stream 0 passed on purpose while
    the harness believes ``S``: fa_copy_f32 and one fa_reduce at n = 5.  The
    harness must report a mismatch; a match means the null stream does wait
    for ``S`` here, and no case of the module proves anything.  The control
    reads allocated memory that holds finite poison: it faults nothing."""
    import ctypes

    from feddct_amd import _lib
    L = _lib.lib
    null = torch.cuda.default_stream()
    numel, n = 4096, 5
    rng = np.random.default_rng(5)
    # fa_copy_f32
    src = torch.from_numpy(rng.standard_normal(numel).astype(np.float32)).cuda()
    dst = torch.full((numel,), -7.0, device="cuda")
    want = src.cpu().numpy()
    ins = [In(src)]

    def copy(st):
        assert L.fa_copy_f32(src.data_ptr(), dst.data_ptr(), numel,
                             ctypes.c_void_p(st.cuda_stream)) == _lib.FA_OK

    # fa_reduce, n = 5, one 4096-float key
    cl = torch.from_numpy(rng.standard_normal((n, numel)).astype(np.float32)).cuda()
    out = torch.full((numel,), -7.0, device="cuda")
    plan = _lib.Plan(np.asarray([(0, numel)], np.int64), numel)
    a32 = _lib.ptr_array([cl.data_ptr() + 4 * numel * i for i in range(n)])
    rins = [In(cl)]

    def reduce(st):
        assert L.fa_reduce(plan.handle, a32, None, n, None, out.data_ptr(), None, 0,
                           ctypes.c_void_p(st.cuda_stream)) == _lib.FA_OK

    for what, call, inputs, o in (("fa_copy_f32", copy, ins, dst), ("fa_reduce", reduce, rins, out)):
        o.fill_(-7.0)
        good = run(arr, S, call, inputs, [o], ("power", what, "on S"))
        ref = good.out[0]
        assert not (ref == -7.0).any(), (what, arr, "the call on S left the sentinel")
        if what == "fa_copy_f32":
            assert np.array_equal(ref, want), (what, arr)
        o.fill_(-7.0)
        bad = run(arr, S, call, inputs, [o], ("power", what, "on stream 0"), call_stream=null)
        assert not np.array_equal(bad.out[0], ref), \
            (what, arr, "harness has no power on this machine: a call launched on stream 0 "
                        "passed for one launched on the side stream")
    torch.cuda.synchronize()
