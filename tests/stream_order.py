"""The staged-call harness of the stream-order tests (test_gpu_stream_order.py, test_gpu_stream_order_side.py).

include/range_hip.h promises that a call is asynchronous on the caller's stream and orders there like any other
work.  A test on an idle device with complete inputs cannot see a launch, memset or copy that sits on another
stream, a read of the caller's buffer deferred behind the call's return, or a hidden synchronisation: nothing else
is running, so everything is in order by accident.  Here the inputs are NOT complete when the call is issued.

A case gives two input sets of the same shapes and dtypes, ``real`` and ``decoy`` - both valid, finite batches - and
``call(*buffers) -> tuple of tensors``.  ``run_staged``:

1. reference: on the default stream, synchronised, ``want = call(real)`` and ``other = call(decoy)``; every output
   tensor of ``want`` must differ from ``other`` (a case that cannot tell the batches apart checks nothing);
2. staging: the buffers hold ``decoy``.  On a fresh stream S, with no host synchronisation between the items: a
   delay kernel of one workgroup, an event ``gate``, copies of ``real`` into the buffers, ``call`` under S, clones
   of its outputs, copies of ``decoy`` back over the buffers, a second ``call``, clones of its outputs;
3. staging condition (``blocks=False``): ``gate.query()`` is False when all of that has been enqueued - the delay
   was still running, so anything that ignored S read decoys, and the call did not block the host.  For a call the
   header states as synchronising (``blocks=True``) the gate is open immediately in front of the first call;
4. verdict: after ``S.synchronize()`` the first clones equal ``want`` and the second ``other``, ``torch.equal``.

Work that ran early (on another stream, not behind S) computes the decoy batch; a read deferred behind the return
sees the decoys copied back in (first call) or whatever follows; a blocked host trips the staging condition.

``control_exposes_stale_read`` turns the harness on itself: a stand-in call issued on a stream that is NOT ordered
behind S must be seen to read the decoys.  With few hardware queues two streams can share one and serialise, which
hides the stale read on that stream; so the default stream and up to three fresh streams - created right behind the
one busy stream, which serves all four tries - are tried and one of them has to expose it.  That aliasing can only HIDE a defect of the library in a given run - work on a wrong stream that
happens to share S's queue runs in order - it can never fail a correct library.

The delay is ``torch.cuda._sleep`` (one workgroup: the one-launch encoder and the fused top-k scan need their whole
grid resident, a chip-filling delay would starve them), calibrated once per process with a pair of events and sized
per case from the warmed call's own host time, 30 ms at the least, 250 ms at the most (``delay_ms_for``).
"""
from __future__ import annotations

import math
import os
import re
import time
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

MIN_DELAY_MS, MAX_DELAY_MS = 30.0, 250.0
#: the staged sequence is two calls and a few copies; the delay is this many times its measured host time
HOST_TIME_FACTOR = 4.0

_rate: Optional[float] = None          # _sleep cycles per millisecond
#: case name -> delay in ms of its last staged run (profiles/NOTES.md quotes these)
DELAYS_USED: Dict[str, float] = {}


class Case(NamedTuple):
    """A row of a case table."""
    name: str
    covers: Tuple[str, ...]                  # the entry points of the headers this case issues on the busy stream
    build: Callable[[], tuple]               # () -> (real, decoy, call)
    blocks: bool = False                     # the header states the call as synchronising


HEADERS = ("range_hip.h", "range_neighbors.h", "range_probe.h", "range_map.h", "range_cluster.h")


def stream_entry_points() -> Dict[str, List[str]]:
    """Per public header the names of the functions it declares with a ``range_stream_t`` parameter, in order
    (needs no GPU: the headers are parsed as text, comments removed)."""
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    found = {}
    for header in HEADERS:
        with open(os.path.join(inc, header)) as f:
            text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        found[header] = [m.group(1) for m in re.finditer(r"\b(range_\w+)\s*\(([^()]*)\)\s*;", text)
                         if re.search(r"\brange_stream_t\b", m.group(2))]
    return found


def sleep_cycles_per_ms(device) -> float:
    """``torch.cuda._sleep`` cycles per millisecond of device time, measured once: the second of two timed sleeps
    (the first pays the kernel's load)."""
    global _rate
    if _rate is None:
        cycles = 20_000_000
        ms = 0.0
        for _ in range(2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(device)
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
        assert ms > 0.0, "the delay kernel took no time"
        _rate = cycles / ms
    return _rate


def delay_ms_for(host_ms: float) -> float:
    """The delay of a case whose staged sequence takes ``host_ms`` of host time: ``HOST_TIME_FACTOR`` times that,
    rounded up to 10 ms, at least ``MIN_DELAY_MS``, at most ``MAX_DELAY_MS``."""
    want = math.ceil(HOST_TIME_FACTOR * host_ms / 10.0) * 10.0
    return float(min(MAX_DELAY_MS, max(MIN_DELAY_MS, want)))


def _clones(outs) -> Tuple[torch.Tensor, ...]:
    if torch.is_tensor(outs):
        outs = (outs,)
    assert len(outs) > 0 and all(torch.is_tensor(o) for o in outs), "a case returns a tuple of tensors"
    return tuple(o.clone() for o in outs)


def _fill(bufs: Sequence[torch.Tensor], src: Sequence[torch.Tensor]) -> None:
    for b, s in zip(bufs, src):
        b.copy_(s, non_blocking=True)


def _same(name: str, what: str, got: Sequence[torch.Tensor], want: Sequence[torch.Tensor], other: Sequence[torch.Tensor]):
    assert len(got) == len(want), f"{name}: {what}: {len(got)} outputs for {len(want)}"
    for i, (g, w, o) in enumerate(zip(got, want, other)):
        if not torch.equal(g, w):
            verdict = "it equals the OTHER batch's result" if torch.equal(g, o) else "it equals neither batch's result"
            raise AssertionError(f"{name}: {what}: output {i} {tuple(g.shape)} {g.dtype} is not the bits of the reference "
                                 f"on the default stream; {verdict}")


def run_staged(name: str, device, real: Sequence[torch.Tensor], decoy: Sequence[torch.Tensor],
               call: Callable[..., Tuple[torch.Tensor, ...]], blocks: bool = False, cold: bool = False,
               want: Optional[Sequence[torch.Tensor]] = None, other: Optional[Sequence[torch.Tensor]] = None) -> float:
    """One case through the harness (module docstring); returns the delay used, in ms.  ``cold``: no reference is
    computed here - ``want`` / ``other`` come from the caller (another context) and the first call this context
    ever sees is the staged one on S (treated as ``blocks``: growth may synchronise)."""
    device = torch.device(device)
    assert len(real) == len(decoy) and len(real) > 0
    for r, d in zip(real, decoy):
        assert r.device == device and d.device == device and r.shape == d.shape and r.dtype == d.dtype, name
        assert r.is_floating_point() is False or bool(torch.isfinite(r).all() and torch.isfinite(d).all()), name
    bufs = [d.clone() for d in decoy]
    host_ms = 0.0
    if cold:
        assert want is not None and other is not None
        blocks = True
    else:
        # 1. the reference, which also warms every workspace to its final size
        torch.cuda.synchronize(device)
        _fill(bufs, real)
        want = _clones(call(*bufs))
        torch.cuda.synchronize(device)
        _fill(bufs, decoy)
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        other = _clones(call(*bufs))              # (the warmed call's own host time, clones included)
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize(device)
    for i, (w, o) in enumerate(zip(want, other)):
        assert w.shape == o.shape and not torch.equal(w, o), \
            f"{name}: output {i} is the same for the real and the decoy batch: the case cannot detect anything"
    delay_ms = delay_ms_for(2.0 * host_ms + 1.0)
    cycles = int(delay_ms * sleep_cycles_per_ms(device))
    DELAYS_USED[name] = delay_ms

    # 2. staging
    S = torch.cuda.Stream(device)
    gate = torch.cuda.Event()
    if not cold:
        # torch's allocator keeps a pool per stream: what the calls and the clones will take from S's pool is put
        # there now, so that no allocation of the staged sequence has to go to the driver
        with torch.cuda.stream(S):
            spare = [torch.empty_like(w) for _ in range(4) for w in want if w.is_cuda]
            spare.append(torch.empty(1 << 20, dtype=torch.uint8, device=device))
            del spare
    torch.cuda.synchronize(device)
    open_before_call = None
    with torch.cuda.stream(S):
        torch.cuda._sleep(cycles)
        gate.record(S)
        _fill(bufs, real)
        if blocks:
            open_before_call = not gate.query()
        first = _clones(call(*bufs))
        _fill(bufs, decoy)
        second = _clones(call(*bufs))
        open_after = not gate.query()
    # 3. the staging condition
    if blocks:
        assert open_before_call, (f"{name}: the staging was too short: the {delay_ms:.0f} ms delay had ended before the "
                                  "call was issued")
    else:
        assert open_after, (f"{name}: the {delay_ms:.0f} ms delay on the caller's stream had ended when the two calls had been "
                            f"enqueued (their host time on an idle device: {2.0 * host_ms:.2f} ms): the call blocked the host, "
                            "or the staging was too short")
    # 4. the verdict
    S.synchronize()
    torch.cuda.synchronize(device)
    _same(name, "first call on the busy stream (inputs copied in behind the delay)", first, want, other)
    _same(name, "second call back to back (decoys copied back in)", second, other, want)
    return delay_ms


def control_exposes_stale_read(device, delay_ms: float = MIN_DELAY_MS) -> List[str]:
    """The harness's own sensitivity: a stand-in call (``x * 2``) issued on a stream that is not ordered behind S
    must read the decoys.  Returns the names of the streams that exposed the stale read (module docstring: with
    few hardware queues some may not)."""
    device = torch.device(device)
    real = torch.arange(1.0, 4097.0, dtype=torch.float64, device=device)
    decoy = -real
    cycles = int(delay_ms * sleep_cycles_per_ms(device))
    exposed = []
    # ONE busy stream, and the fresh candidates created right behind it: where the runtime deals its hardware queues
    # out in turn, the next three streams sit on the three other queues of four (a new S per candidate would move
    # in step with the candidates and could alias every one of them)
    S = torch.cuda.Stream(device)
    candidates = [("default stream", torch.cuda.default_stream(device))]
    candidates += [(f"fresh stream {i + 1}", torch.cuda.Stream(device)) for i in range(3)]
    for label, T in candidates:
        buf = decoy.clone()
        with torch.cuda.stream(T):
            spare = torch.empty_like(buf)
            del spare
        torch.cuda.synchronize(device)
        gate = torch.cuda.Event()
        with torch.cuda.stream(S):
            torch.cuda._sleep(cycles)
            gate.record(S)
            buf.copy_(real, non_blocking=True)
        with torch.cuda.stream(T):                # the defect under test: the "library" ignores the caller's stream
            out = buf * 2.0
        still_open = not gate.query()
        S.synchronize()
        T.synchronize()
        torch.cuda.synchronize(device)
        assert torch.equal(buf, real)
        if still_open and torch.equal(out, decoy * 2.0):
            exposed.append(label)
        else:
            assert torch.equal(out, real * 2.0) or not still_open, f"control on the {label}: neither batch's result"
    return exposed
