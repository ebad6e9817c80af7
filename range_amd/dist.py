"""Row-sharded bank across the GPUs of one node: one process per GPU, torch.distributed
(backend "nccl" = RCCL over xGMI).

The reference has no distributed code; this is the north-star layout: rank r
holds bank rows [r*N/W, (r+1)*N/W) and serves its own B queries; the soft-attention over N
decomposes exactly over row shards:

    1. encode the local queries (kernel A)                       no communication
    2. all-gather of the query operands e32 (B,256) and xq (B,4): W*B*1040 B per rank
    3. pass 1 on the local shard for ALL W*B queries -> softmax statistics (m, l) with the
       constant shift m = tau*log2(e) (unit-vector logits), so the l of disjoint shards ADD
       (temperatures above 43: m is the shard's largest scaled logit)
    4. all-gather of the statistics (W*B,4) + merge in rank order (an exact log-sum-exp merge; with
       the same m the l add: a fixed order, where an all-reduce's would depend on an element's
       place in the buffer)
    5. pass 2 on the local shard with the GLOBAL statistics -> partial (W*B,1024) f32; partials
       of different shards simply add because the weights are already globally normalised
    6. all-to-all: rank r receives the W partial slices of ITS queries (one direct transfer per
       peer, so all 7 xGMI links of a GPU carry 1/7 of the traffic each - not a ring)
    7. finalize: fixed-order sum of the W slices + pack with e64 -> (B,1280) float64

Steps 2-7 run per query CHUNK and every collective is asynchronous (RCCL's own stream): the
gathers of all chunks are issued behind the encoder, pass 1 of chunk c runs while the gather of
chunk c+1 and the statistics of chunk c-1 travel, pass 2 of chunk c while the exchange of chunk c-1
travels.  Exposed on the compute stream: the first chunk's gather and the last chunk's exchange.
Pass 1 keeps the logits of all chunks in ONE workspace (range_scan_stats_at), every chunk with the
same bank-split count, so a query's statistics - and the result - do not depend on the chunking.

The top-k side channel merges per-shard candidate lists with ONE all-gather (north star).

Per-GPU work is B_total * N / W = B * N: adding GPUs adds queries at constant time per step
(weak scaling).  The engine is duck-typed (``ShardEngine`` below; ``_native.HipEngine``) so that the
collective logic can be exercised on CPU with the gloo backend and a checker engine in tests.
"""
from __future__ import annotations

import os
from functools import partial
from typing import Optional, Protocol, Tuple

import torch
import torch.distributed as dist

from .range import attend_any, range_model, sweep_plan


def shard_rows(n_rows: int, world_size: int, rank: int) -> Tuple[int, int]:
    """Contiguous, balanced row range of ``rank``."""
    return (n_rows * rank) // world_size, (n_rows * (rank + 1)) // world_size


class ShardEngine(Protocol):
    """What ``ShardedRange`` calls on its engine, over THIS rank's bank rows (``_native.HipEngine``
    documents each; B = queries of the call, f32 / f64 tensors on the engine's device)."""

    def encode(self, lonlat): ...                      # (B,2) f64 -> e64 (B,256) f64, e32 (B,256), xq (B,4)
    def p1_splits(self, n_queries: int) -> int: ...    # bank splits pass 1 chooses for n_queries
    def scan_stats_at(self, e32, xq, tau_sem, tau_geo, first_query, total_queries, n_splits=0): ...   # -> (B,4)
    def kept_queries(self) -> int: ...                 # queries whose logits the current scan kept
    def merge_stats(self, parts): ...                  # (W,B,4) -> (B,4), rank order
    def attend(self, e32, xq, tau_sem, tau_geo, beta, stats): ...              # -> (B,1024) partial
    def attend_kept(self, first_query, xq, tau_sem, tau_geo, beta, stats): ...  # the same, from kept logits
    def blend(self, G, H, beta): ...                   # (1-beta) G + beta H, (B,1024)
    def finalize(self, partials, e64, out=None): ...   # (W,B,1024), (B,256) f64 -> (B,1280) f64 (into ``out``)
    def topk_stream(self, e32, k: int): ...            # -> values (B,k) f32, global rows (B,k) i64
    def merge_topk(self, vals, idxs): ...              # (W,B,k) each -> (B,k) each


class SweepShardEngine(ShardEngine, Protocol):
    """What a temperature sweep (``ShardedRange.sweep(..., temps=, geo_temps=)``) calls in addition."""

    def stats_kept(self, first_query, xq, taus, n_splits=0): ...   # (P,B,4): the statistics at P (tau_sem, tau_geo) pairs, from the kept logits


def start_collective(kind: str, src: torch.Tensor, group=None, dst: Optional[torch.Tensor] = None,
                     alloc=None):
    """Start the collective ``kind`` of ``src`` asynchronously: "all_gather_into_tensor" ((n, ...) ->
    (W*n, ...), rank-major: the concatenation form both RCCL and gloo accept) or "all_to_all_single"
    (W equal slices, one direct transfer per peer).  Device tensors over the gloo backend (several
    ranks sharing one GPU in tests, or a box without RCCL) travel as host copies; RCCL moves device
    memory directly.  Received into ``dst`` (on ``src``'s device) when given, else into
    ``alloc(shape, dtype, device)`` (default: a new tensor) on the device the collective runs on.
    Returns (work, landed): once ``work.wait()`` has returned, ``landed()`` is the received tensor
    on ``src``'s device (it also keeps the operands alive until then)."""
    staged = src.is_cuda and dist.get_backend(group) == "gloo"
    send = src.cpu() if staged else src.contiguous()
    recv = dst
    if dst is None or staged:
        shape = tuple(src.shape) if dst is None else tuple(dst.shape)
        if dst is None and kind == "all_gather_into_tensor":
            shape = (dist.get_world_size(group) * shape[0],) + shape[1:]
        recv = (alloc or (lambda s, t, d: torch.empty(s, dtype=t, device=d)))(shape, src.dtype, send.device)
    work = getattr(dist, kind)(recv, send, group=group, async_op=True)

    def landed(_keep=send):
        if dst is None:
            return recv.to(src.device)
        return dst if recv is dst else dst.copy_(recv)
    return work, landed


def pack_topk(tv: torch.Tensor, ti: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Top-k candidates as ONE float32 buffer ``out`` (n,k,3): the values and the int64 rows' bit
    patterns (2 x f32) - one collective instead of two."""
    out[:, :, 0] = tv
    out[:, :, 1:] = ti.view(torch.float32).reshape(tuple(tv.shape) + (2,))
    return out


def unpack_topk(buf: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(..., k, 3) packed candidates -> contiguous values (..., k) float32 and rows (..., k) int64."""
    return buf[..., 0].contiguous(), buf[..., 1:].contiguous().view(torch.int64).reshape(buf.shape[:-1])


class ShardedRange:
    """RANGE / RANGE+ forward over a row-sharded bank.  ``engine`` holds THIS rank's rows."""

    #: queries per rank and chunk below which a forward is not split further.  Chunks buy overlap -
    #: the statistics of chunk c travel under pass 1 of chunk c+1, its exchange under pass 2 of chunk
    #: c+1, so only the first gather and the last exchange are exposed - and cost launches: what a rank
    #: of 8 computes for BASELINE's 10 000-query batch (1 250 own, 10 000 scanned against 12 500 rows;
    #: tools/shard_emulate.py --chunks k 8, round 4) takes 2.885 ms as one chunk, 3.011 ms as two,
    #: 3.119 ms as four.  Default: TWO chunks from 1 024 queries per rank (three blocking
    #: collectives -> one gather + half an exchange exposed), four from 8 192 (the weak mode, where a
    #: rank ships >= 8 MB per peer and chunk)
    min_chunk = 512

    def __init__(self, engine, model_name: str = "RANGE+", beta: Optional[float] = 0.5,
                 group=None, n_chunks: Optional[int] = None, *, tau_sem: Optional[float] = None,
                 tau_geo: Optional[float] = None):
        # (tau_sem / tau_geo: other temperatures than the reference's defaults - the same on every rank;
        # above 43 every shard's pass 1 keeps a running maximum and the shards' m differ: merge_stats is
        # an exact log-sum-exp merge either way)
        self.tau_sem, self.tau_geo, _, _ = range_model(model_name, tau_sem, tau_geo)
        self.beta = float(beta) if self.tau_geo else 1.0        # (RANGE: the semantic retrieval alone)
        self.engine: ShardEngine = engine
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.n_chunks = n_chunks   # None: 2 or 4 chunks (by batch size) when there is a peer to exchange with
        # gathered / chunk-major / receive buffers: one per name, sized to the largest request seen
        # (a step then makes no allocation of its own besides the engine's outputs)
        self._bufs = {}
        self._timing = False
        self._events = {}
        #: pass 1 per chunk with its collectives overlapped; False: one pass 1 over all scanned queries
        #: between a blocking gather and a blocking all-reduce (A/B, tests)
        self.pass1_chunked = True
        #: RANGE_DIST_BLOCKING=1: every collective is waited for where it is issued (no overlap with
        #: compute, one pass 1 over all scanned queries) - the escape hatch for bisecting a hang or a
        #: wrong result on a backend the overlapped schedule has not met (it has run over gloo and
        #: the in-process test backend, and over RCCL with ONE rank; with more than one rank it has not executed)
        self.blocking = os.environ.get("RANGE_DIST_BLOCKING", "0") == "1"
        if self.blocking:
            self.pass1_chunked = False
        #: bytes this rank SENT / RECEIVED per kind of collective since ``reset_bytes()`` (payload
        #: sizes; "results" = what the batch drivers move to rank 0, range.ShardedLocationEncoder)
        self.bytes_sent = {}
        self.bytes_received = {}

    def reset_bytes(self):
        self.bytes_sent, self.bytes_received = {}, {}

    def _count(self, kind: str, sent: int, received: int):
        self.bytes_sent[kind] = self.bytes_sent.get(kind, 0) + int(sent)
        self.bytes_received[kind] = self.bytes_received.get(kind, 0) + int(received)

    def _buf(self, name: str, shape, dtype, device) -> torch.Tensor:
        """One flat buffer per (name, dtype, device), grown to the largest request seen; a request is
        a view of its head.  (A buffer per distinct shape would grow without bound under varying
        batch sizes: ragged last batches, a serving loop.)"""
        key = (name, dtype, str(device))
        n = 1
        for d in shape:
            n *= int(d)
        t = self._bufs.get(key)
        if t is None or t.numel() < n:
            t = self._bufs[key] = torch.empty(max(n, 1), dtype=dtype, device=device)
        return t[:n].view(tuple(shape))

    # -- exposed communication time ------------------------------------------------------------
    def comm_timing(self, on: bool):
        """``comm_timing(True)`` starts measuring, ``comm_timing(False)`` stops and returns the
        milliseconds the COMPUTE stream spent blocked on collectives since, per kind - a dict
        {"gather", "reduce", "exchange", "total"} (event pairs around every point where the stream
        waits for one: the time a collective - including the wait for the slowest peer - is not
        hidden behind this rank's kernels).  None without a GPU."""
        if on:
            self._events, self._timing = {}, torch.cuda.is_available()
            return None
        if not self._timing:
            return None
        self._timing = False
        torch.cuda.synchronize()
        ms = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in self._events.items()}
        for k in ("gather", "reduce", "exchange"):
            ms.setdefault(k, 0.0)
        ms["total"] = sum(ms.values())
        self._events = {}
        return ms

    def _blocked(self, kind: str, fn):
        """Run ``fn`` (something that makes the current stream wait for a collective) between two
        events on the current stream."""
        if not self._timing:
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        self._events.setdefault(kind, []).append((a, b))
        return r

    def _start(self, kind: str, src: torch.Tensor, key: str, timed: Optional[str],
               dst: Optional[torch.Tensor] = None, name: Optional[str] = None):
        """The one way a collective is issued here (``start_collective``): counts its payload under
        ``key``, starts it asynchronously - received into ``dst``, else into the buffer ``name`` - and
        returns the function that makes the current stream wait for it and yields the received tensor
        on ``src``'s device.  The wait runs under ``_blocked(timed, ...)`` (``timed=None``: untimed,
        the caller times it).  ``blocking``: waited for here, where it is issued; the returned
        function then only lands the result."""
        nb = src.numel() * src.element_size() // (self.world if kind == "all_to_all_single" else 1)
        self._count(key, nb * (self.world - 1), nb * (self.world - 1))
        work, landed = start_collective(kind, src, self.group, dst, name and partial(self._buf, name))
        wait = (lambda: self._blocked(timed, work.wait)) if timed else work.wait
        if self.blocking:
            wait()
            return landed

        def result():
            wait()
            return landed()
        return result

    def _gather(self, t: torch.Tensor, name: str) -> torch.Tensor:
        """Blocking all-gather of ``t`` -> (W, *t.shape); the time from its issue on counts as exposed."""
        out = self._blocked("gather", lambda: self._start("all_gather_into_tensor", t, "gather", None,
                                                          name="gather:" + name)())
        return out.reshape((self.world,) + tuple(t.shape))

    def _stats_start(self, stats: torch.Tensor, name: str):
        """Start the all-gather of a chunk's statistics (n,4) and return the function that waits for
        it and merges the W shards' rows in rank order (engine.merge_stats: same shift m, the l add).
        Not an all-reduce: a ring or tree sums an element in an order that depends on where it sits
        in the buffer, so a query's l - and with it the result - would change in the last bit with
        the batch it travels in; the fixed-order merge keeps the sharded result independent of the
        chunking and of the collective algorithm (16 B per scanned query to every peer, one small
        kernel).  Counted and timed under the key "reduce" (what it replaces); the time is the
        wait for the collective alone, not the merge kernel behind it."""
        got = self._start("all_gather_into_tensor", stats, "reduce", "reduce", name="gather:" + name)
        return lambda: self.engine.merge_stats(got().view((self.world,) + tuple(stats.shape)))

    def _exchange(self, part: torch.Tensor, name: str):
        """Start the all-to-all of a chunk's partials (asynchronous, so that the exchange of this
        chunk overlaps pass 2 of the next); returns the function that waits for it and yields the W
        slices received."""
        return self._start("all_to_all_single", part, "exchange", "exchange", name="recv:" + name)

    def _gather_queries(self, lonlat: torch.Tensor):
        """Encode the own queries and gather every rank's scan operands: e32 (B,256) and xq (B,4)
        travel as ONE packed (B,260) buffer - at these sizes a collective costs its latency, not
        its bytes.  Returns e64 (own) and the (W*B,256) / (W*B,4) column views of the gathered
        buffer (strided: ``_chunk_major`` lays them out for the scan)."""
        e64, e32, xq = self.engine.encode(lonlat)
        W, B, d = self.world, lonlat.shape[0], e32.shape[1]
        packed = self._buf("pack:q", (B, d + xq.shape[1]), e32.dtype, e32.device)
        packed[:, :d] = e32
        packed[:, d:] = xq
        allq = self._gather(packed, "q").reshape(W * B, d + xq.shape[1])
        return e64, allq[:, :d], allq[:, d:]

    def _chunk_major(self, t_all: torch.Tensor, chunks, name: str) -> torch.Tensor:
        """(W*B, d) in rank-major order (a column view of the gathered buffer) -> contiguous,
        chunk-major order: rows [lo,hi) of EVERY rank's queries form one chunk, ordered by owner
        rank - a contiguous range of the scanned batch whose partial is again W equal slices, one
        per destination."""
        out = self._buf("cm:" + name, t_all.shape, t_all.dtype, t_all.device)
        if len(chunks) == 1:
            out.copy_(t_all)
            return out
        W = self.world
        B = t_all.shape[0] // W
        v = t_all.view(W, B, -1)
        for lo, hi in chunks:
            out[W * lo:W * hi].view(W, hi - lo, -1).copy_(v[:, lo:hi])
        return out

    def _chunk_bounds(self, B: int):
        """Row ranges [lo,hi) of a rank's queries per chunk.  Boundaries are multiples of 64 (the
        query-tile size: a chunk then starts on a tile of the kept logits)."""
        W = self.world
        n_chunks = self.n_chunks if self.n_chunks else ((4 if B >= 8192 else 2) if W > 1 else 1)
        n_chunks = max(1, min(n_chunks, B // self.min_chunk))
        cuts = sorted({min(B, ((B * c) // n_chunks + 32) // 64 * 64) for c in range(1, n_chunks)})
        bounds = [0] + [c for c in cuts if 0 < c < B] + [B]
        return list(zip(bounds[:-1], bounds[1:]))

    def _scan(self, lonlat: torch.Tensor):
        """Steps 1-4 for this rank's (B,2) queries.  Returns (e64 of the own queries, e32 and xq of
        ALL W*B scanned queries in chunk-major order, the chunk bounds, one function per chunk that
        returns the chunk's GLOBAL statistics once the current stream may read them, and whether pass 2
        finds the scan's logits kept)."""
        W, B = self.world, lonlat.shape[0]
        eng = self.engine
        chunks = self._chunk_bounds(B)
        if not self.pass1_chunked:
            e64, e32_all, xq_all = self._gather_queries(lonlat)
            e32_all = self._chunk_major(e32_all, chunks, "e32")
            xq_all = self._chunk_major(xq_all, chunks, "xq")
            n_max = W * max(hi - lo for lo, hi in chunks)
            # (the same bank splits as the chunked form: bit-identical statistics)
            stats_local = eng.scan_stats_at(e32_all, xq_all, self.tau_sem, self.tau_geo, 0, W * B,
                                            n_splits=eng.p1_splits(n_max))
            stats = self._stats_start(stats_local, "stats")()
            getters = [(lambda lo=lo, hi=hi: stats[W * lo:W * hi]) for lo, hi in chunks]
            return e64, e32_all, xq_all, chunks, getters, eng.kept_queries() == W * B
        e64, e32, xq = eng.encode(lonlat)
        total = W * B
        e32_all = self._buf("cm:e32", (total, e32.shape[1]), e32.dtype, e32.device)
        xq_all = self._buf("cm:xq", (total, xq.shape[1]), xq.dtype, xq.device)
        # every chunk's gather is issued now: a chunk's rows of all ranks land rank-major in rows
        # [W lo, W hi) - the chunk-major order of the scan, no copy.  (Their waits are timed HERE, in
        # the loop below; a ``blocking`` gather has been waited for at its issue, untimed)
        landed = [tuple(self._start("all_gather_into_tensor", t[lo:hi], "gather", None, dst=t_all[W * lo:W * hi])
                        for t, t_all in ((e32, e32_all), (xq, xq_all))) for lo, hi in chunks]
        n_splits = eng.p1_splits(W * max(hi - lo for lo, hi in chunks))
        getters = []
        for (lo, hi), (we, wx) in zip(chunks, landed):
            self._blocked("gather", we)
            self._blocked("gather", wx)
            first, n = W * lo, W * (hi - lo)
            st = eng.scan_stats_at(e32_all[first:first + n], xq_all[first:first + n], self.tau_sem, self.tau_geo,
                                   first, total, n_splits=n_splits)
            getters.append(self._stats_start(st, f"stats{len(getters)}"))
        return e64, e32_all, xq_all, chunks, getters, eng.kept_queries() == total

    def _topk_start(self, e32_all: torch.Tensor, chunks, k: int):
        """The top-k side channel of a forward (``forward(..., topk=k)``): this shard's top-k for ALL
        scanned queries - their e-hat is gathered already, in chunk-major order - and the start of
        the ONE all-gather of the packed candidates (north star); returns the function that waits for
        it and merges this rank's OWN queries' W lists (global rows, ties to the lower row)."""
        W, total = self.world, e32_all.shape[0]
        # (the keys-only scan: it leaves the logits pass 1 kept for pass 2 alone)
        tv, ti = self.engine.topk_stream(e32_all, k)
        packed = pack_topk(tv, ti, self._buf("pack:topk", (total, k, 3), torch.float32, tv.device))
        # (counted as "topk"; its wait is timed with the gathers)
        got = self._start("all_gather_into_tensor", packed, "topk", "gather", name="gather:fwd_topk")

        def merged():
            a = got().view(W, total, k, 3)
            # this rank's rows of the chunk-major order: chunk (lo,hi) holds them at W lo + rank (hi - lo)
            own = torch.cat([a[:, W * lo + self.rank * (hi - lo):W * lo + (self.rank + 1) * (hi - lo)] for lo, hi in chunks], dim=1)
            return self.engine.merge_topk(*unpack_topk(own))
        return merged

    @torch.no_grad()
    def forward(self, lonlat: torch.Tensor, out: Optional[torch.Tensor] = None, topk: Optional[int] = None):
        """lonlat: this rank's (B,2) float64 queries (same B on every rank).
        Returns this rank's (B,1280) float64 embeddings (device tensor; ``out`` when given: the
        chunks are finalized straight into its rows).  ``topk=k``: returns (embeddings, values (B,k)
        float32, global bank rows (B,k) int64) - the top-k side channel from the same call: the
        queries are encoded and gathered ONCE, every shard scans the gathered e-hat behind its pass 1,
        the candidates travel in one all-gather under pass 2."""
        W = self.world
        e64, e32_all, xq_all, chunks, stats_of, kept = self._scan(lonlat)
        topk_of = self._topk_start(e32_all, chunks, int(topk)) if topk else None
        pending = []
        for ci, (lo, hi) in enumerate(chunks):
            first, n = W * lo, W * (hi - lo)
            part = attend_any(self.engine, kept, first, e32_all[first:first + n], xq_all[first:first + n],
                              self.tau_sem, self.tau_geo, self.beta, stats_of[ci]())
            pending.append((self._exchange(part, f"fwd{ci}"), lo, hi))
        if out is None:
            out = torch.empty((lonlat.shape[0], e64.shape[1] + 1024), dtype=torch.float64, device=e64.device)
        for received, lo, hi in pending:
            self.engine.finalize(received().reshape(W, hi - lo, -1), e64[lo:hi], out=out[lo:hi])
        if topk_of is not None:
            tv, ti = topk_of()
            return out, tv, ti
        return out

    __call__ = forward

    #: scanned queries (all ranks') per outer step of ``embed`` / ``embed_sweep``: bounds the
    #: per-rank workspace like LocationEncoder.chunk_size does on one GPU (kept logits: 4 B x
    #: scanned queries x local rows; split slabs: splits x scanned queries x 4 KB)
    scan_chunk = 16384

    def _max_over_ranks(self, n: int, device) -> int:
        t = torch.tensor([n], dtype=torch.int64,
                         device=device if dist.get_backend(self.group) != "gloo" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        return int(t.item())

    def _steps(self, lonlat: torch.Tensor, chunk: Optional[int], b_max: Optional[int] = None):
        """Outer steps of a ragged job: every rank brings its OWN number of queries (0 allowed); the
        ranks agree on the largest count (one scalar all-reduce), walk it in steps of ``chunk``
        queries per rank and pad their share of a step to the step's size with copies of a dummy
        location - every collective of a step then has the same shape on every rank.  Yields
        (lo, n_own, padded (c,2) tensor)."""
        if lonlat.dim() != 2 or lonlat.shape[1] != 2:
            raise ValueError(f"lonlat must be (B,2) (lon,lat) degrees, got {tuple(lonlat.shape)}")
        B = lonlat.shape[0]
        if b_max is None:      # (a caller that knows every rank brings the same count passes it: no collective)
            b_max = self._max_over_ranks(B, lonlat.device)
        elif B > b_max:
            # (rows beyond b_max would never be computed; b_max must be the SAME on every rank of the
            # group - the steps' collectives are shaped by it - and cover every rank's count)
            raise ValueError(f"this rank brings {B} queries but b_max={b_max}")
        if chunk is None:
            chunk = max(64, self.scan_chunk // self.world // 64 * 64)
        chunk = max(1, int(chunk))
        for lo in range(0, b_max, chunk):
            c = min(chunk, b_max - lo)
            own = lonlat[lo:lo + c]
            n_own = own.shape[0]
            if n_own < c:
                pad = self._buf("pad:q", (c, 2), lonlat.dtype, lonlat.device)
                pad.zero_()
                pad[:n_own] = own
                own = pad
            yield lo, n_own, own.contiguous()

    @torch.no_grad()
    def embed(self, lonlat: torch.Tensor, chunk: Optional[int] = None,
              out: Optional[torch.Tensor] = None, b_max: Optional[int] = None, topk: Optional[int] = None):
        """The product entry of the row-sharded path: this rank's (B,2) queries -> its (B,1280)
        float64 embeddings (device tensor), for ANY per-rank B (ragged across ranks, zero on some),
        in outer steps of ``chunk`` queries per rank (default: ``scan_chunk`` scanned queries per
        step).  Collective: every rank of the group must call it.  ``b_max``: the largest per-rank
        count, when the caller knows it (equal counts: ``b_max=B``) - saves the scalar all-reduce.
        ``topk=k``: returns (embeddings, values (B,k), global rows (B,k)) - see ``forward``."""
        B = lonlat.shape[0]
        if out is None:
            out = torch.empty((B, 1280), dtype=torch.float64, device=lonlat.device)
        if topk:
            tv = torch.empty((B, topk), dtype=torch.float32, device=lonlat.device)
            ti = torch.empty((B, topk), dtype=torch.int64, device=lonlat.device)
        for lo, n_own, q in self._steps(lonlat, chunk, b_max):
            if topk:
                res, v, i = self.forward(q, topk=topk)
                if n_own:
                    out[lo:lo + n_own], tv[lo:lo + n_own], ti[lo:lo + n_own] = res[:n_own], v[:n_own], i[:n_own]
                continue
            if n_own == q.shape[0]:
                self.forward(q, out=out[lo:lo + n_own])      # (no padding: straight into the result)
                continue
            res = self.forward(q)
            if n_own:
                out[lo:lo + n_own] = res[:n_own]
        return (out, tv, ti) if topk else out

    @torch.no_grad()
    def embed_sweep(self, lonlat: torch.Tensor, betas, chunk: Optional[int] = None,
                    out: Optional[torch.Tensor] = None, b_max: Optional[int] = None, *, temps=None,
                    geo_temps=None) -> torch.Tensor:
        """``embed`` for several beta values at once (one pass 1 and two passes 2 per step whatever
        the number of betas): (len(betas), B, 1280) float64 on the device.  ``temps`` / ``geo_temps``:
        the temperature sweep of ``sweep`` - (T, G, nb, B, 1280), RANGE: (T, B, 1280)."""
        plan = self._sweep_plan(betas, temps, geo_temps)
        lead = (len([float(b) for b in betas]),) if plan is None else plan.lead
        B = lonlat.shape[0]
        if out is None:
            out = torch.empty(lead + (B, 1280), dtype=torch.float64, device=lonlat.device)
        for lo, n_own, q in self._steps(lonlat, chunk, b_max):
            res = self.sweep(q, betas, temps=temps, geo_temps=geo_temps)
            if n_own:
                out[..., lo:lo + n_own, :] = res[..., :n_own, :]
        return out

    @torch.no_grad()
    def embed_topk(self, lonlat: torch.Tensor, k: int = 16, chunk: Optional[int] = None):
        """``topk`` for ragged per-rank batches: (values (B,k) f32, global indices (B,k) i64)."""
        B = lonlat.shape[0]
        tv = torch.empty((B, k), dtype=torch.float32, device=lonlat.device)
        ti = torch.empty((B, k), dtype=torch.int64, device=lonlat.device)
        for lo, n_own, q in self._steps(lonlat, chunk):
            v, i = self.topk(q, k)
            if n_own:
                tv[lo:lo + n_own] = v[:n_own]
                ti[lo:lo + n_own] = i[:n_own]
        return tv, ti

    def _sweep_plan(self, betas, temps, geo_temps):
        name = "RANGE+" if self.tau_geo > 0.0 else "RANGE"
        return sweep_plan(name, betas, temps, geo_temps, self.tau_sem, self.tau_geo or None, self.beta)

    @torch.no_grad()
    def sweep(self, lonlat: torch.Tensor, betas=None, temps=None, geo_temps=None) -> torch.Tensor:
        """RANGE+ embeddings of this rank's queries for several beta values (BASELINE config
        "beta sweep ... 8xMI355X"): one pass 1, per chunk TWO passes 2 on its kept logits (beta = 1:
        the semantic retrieval H, beta = 0: the geographic G), two exchanges, then one blend
        (range.py:238, applied per shard partial - the blend is linear) + finalize per beta.
        Returns (len(betas), B, 1280) float64 on the device.

        ``temps`` / ``geo_temps`` (``range.sweep_plan``: the pairing rule and the result shapes of
        ``LocationEncoder.sweep``): a temperature sweep from the same ONE pass 1.  Per chunk the shard's
        statistics of every pair come from its kept logits (``stats_kept``, with the bank splits of the
        scan) and travel in ONE all-gather - (P n, 4) rows: the merge is row-wise -, then one pass 2 and
        one exchange per semantic and per geographic temperature, a blend + finalize per grid point.
        (T, G, nb, B, 1280); RANGE: (T, B, 1280).  Logits not kept: ``scan_stats_at`` per pair."""
        plan = self._sweep_plan(betas, temps, geo_temps)
        if plan is not None:
            return self._temperature_sweep(lonlat, plan)
        if self.tau_geo <= 0.0:
            raise ValueError("sweep() is defined for RANGE+ only")
        betas = [float(b) for b in betas]
        W, B = self.world, lonlat.shape[0]
        e64, e32_all, xq_all, chunks, stats_of, kept = self._scan(lonlat)
        pending = []
        for ci, (lo, hi) in enumerate(chunks):
            first, n = W * lo, W * (hi - lo)
            sl = slice(first, first + n)
            st = stats_of[ci]()
            parts = [attend_any(self.engine, kept, first, e32_all[sl], xq_all[sl], self.tau_sem, self.tau_geo, b, st)
                     for b in (1.0, 0.0)]
            pending.append(([self._exchange(p, f"sweep{ci}:{j}") for j, p in enumerate(parts)], lo, hi))
        out = torch.empty((len(betas), B, e64.shape[1] + 1024), dtype=torch.float64,
                          device=e64.device)
        for (got_h, got_g), lo, hi in pending:
            rH, rG = got_h(), got_g()
            e = e64[lo:hi].contiguous()
            for j, b in enumerate(betas):
                mix = self.engine.blend(rG, rH, b)                   # (W*n, 1024): per-shard partials
                out[j, lo:hi] = self.engine.finalize(mix.reshape(W, hi - lo, mix.shape[1]), e)
        return out

    def _temperature_sweep(self, lonlat: torch.Tensor, plan) -> torch.Tensor:
        W, B = self.world, lonlat.shape[0]
        eng = self.engine
        e64, e32_all, xq_all, chunks, stats_of, kept = self._scan(lonlat)
        total = W * B
        n_splits = eng.p1_splits(W * max(hi - lo for lo, hi in chunks))      # (what _scan gave every chunk)
        P, T = len(plan.pairs), len(plan.temps)
        pending = []
        for ci, (lo, hi) in enumerate(chunks):
            first, n = W * lo, W * (hi - lo)
            sl = slice(first, first + n)
            stats_of[ci]()                                   # (the scan's own statistics: not used, their collective is drained)
            if kept:
                local = eng.stats_kept(first, xq_all[sl], plan.pairs, n_splits=n_splits)
            else:
                local = torch.stack([eng.scan_stats_at(e32_all[sl], xq_all[sl], ts, tg, first, total, n_splits=n_splits)
                                     for ts, tg in plan.pairs])
            # ONE all-gather for the statistics of all pairs: rows (pair, query)
            st = self._stats_start(local.reshape(P * n, 4), f"sweep_stats{ci}")().view(P, n, 4)
            parts = [attend_any(eng, kept, first, e32_all[sl], xq_all[sl], ts, tg, 1.0 if p < T else 0.0, st[p].contiguous())
                     for p, (ts, tg) in enumerate(plan.pairs)]
            pending.append(([self._exchange(part, f"tsweep{ci}:{j}") for j, part in enumerate(parts)], lo, hi))
        out = torch.empty(plan.lead + (B, e64.shape[1] + 1024), dtype=torch.float64, device=e64.device)
        for gots, lo, hi in pending:
            heads = [g() for g in gots]
            e = e64[lo:hi].contiguous()
            for ti in range(T):
                if not plan.geo_temps:                       # RANGE: the semantic retrieval alone
                    out[ti, lo:hi] = eng.finalize(heads[ti].reshape(W, hi - lo, -1), e)
                    continue
                for gi in range(len(plan.geo_temps)):
                    for bi, b in enumerate(plan.betas):
                        mix = eng.blend(heads[T + gi], heads[ti], b)             # (W*n, 1024): per-shard partials
                        out[ti, gi, bi, lo:hi] = eng.finalize(mix.reshape(W, hi - lo, mix.shape[1]), e)
        return out

    @torch.no_grad()
    def topk(self, lonlat: torch.Tensor, k: int = 16):
        """Global top-k (semantic cosine similarity) for this rank's queries: per-shard top-k,
        one all-gather of the candidates, k-way merge."""
        W, B = self.world, lonlat.shape[0]
        _, e32_all, _ = self._gather_queries(lonlat)
        # the HBM-streaming kernel: faster than pass 1's own top-k at every batch size
        tv, ti = self.engine.topk_stream(e32_all.contiguous(), k)
        packed = pack_topk(tv, ti, self._buf("pack:topk", (W * B, k, 3), torch.float32, tv.device))
        allp = self._gather(packed, "topk")                                    # the ONE all-gather
        return self.engine.merge_topk(*unpack_topk(allp[:, self.rank * B:(self.rank + 1) * B]))


def make_layout(row_shards: int, group=None):
    """The 2-D layout R x Q of a W-rank job (W = R Q): the bank is row-sharded over R ranks - a SHARD
    GROUP: ranks g R .. g R + R - 1 - and there are Q such groups, each a full copy of the bank serving
    its own queries.  R = W is the north-star layout (one group, every collective spans the node);
    R = 1 is the query-sharded control (no collective on the data path); in between the collectives
    span R ranks only, the all-to-all is (R - 1) transfers per rank, a shard has N / R rows (pass 2
    keeps its whole-round efficiency on bigger shards) and a rank scans R times its own queries
    instead of W times.  With the default group (``group=None``) every rank of the job must call
    this: the sub-groups are created collectively, each rank entering every ``new_group``.  With a
    sub-group of the job as ``group`` only ITS ranks need to call (they cannot make the other
    ranks enter ``new_group``): each creates just its own shard group with torch's local
    synchronisation.  Returns (shard_group, shard_index, query_group_index)."""
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    R = int(row_shards)
    if R < 1 or world % R:
        raise ValueError(f"row_shards={row_shards} does not divide the {world} ranks")
    if R == world:
        return group, rank, 0
    if group is None or group is dist.group.WORLD:
        ranks = list(range(world))
        mine = None
        for g in range(world // R):
            sub = dist.new_group(ranks=ranks[g * R:(g + 1) * R])
            if rank // R == g:
                mine = sub
        return mine, rank % R, rank // R
    ranks = dist.get_process_group_ranks(group)
    g = rank // R
    try:
        mine = dist.new_group(ranks=ranks[g * R:(g + 1) * R], use_local_synchronization=True)
    except TypeError as ex:       # (a torch without local synchronisation: every rank of the JOB would have to call)
        raise RuntimeError("row_shards < group size over a non-default process group needs a torch whose "
                           "new_group() takes use_local_synchronization") from ex
    return mine, rank % R, rank // R


#: seconds a collective (and the rendezvous) may take before the process group gives up - torch's
#: default is 600 s, the whole budget of a benchmark run: a rank that never arrives must cost two
#: minutes, not the job.  RANGE_DIST_TIMEOUT_S overrides.  Over RCCL the watchdog thread of
#: ProcessGroupNCCL aborts the communicator and ends the process when a collective exceeds it
#: (TORCH_NCCL_ASYNC_ERROR_HANDLING's default); over gloo the waiting call raises.  Either way every
#: rank of a job whose peer hangs exits non-zero within this bound.
DEFAULT_TIMEOUT_S = 120.0


def dist_timeout_s(timeout_s: Optional[float] = None) -> float:
    if timeout_s is not None:
        return float(timeout_s)
    return float(os.environ.get("RANGE_DIST_TIMEOUT_S", DEFAULT_TIMEOUT_S))


def init_from_env(backend: Optional[str] = None, timeout_s: Optional[float] = None,
                  attempt: Optional[int] = None) -> Tuple[int, int, int]:
    """Initialise torch.distributed from RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* (torchrun).

    ``timeout_s``: the process group's timeout (default ``DEFAULT_TIMEOUT_S`` = 120 s, or
    RANGE_DIST_TIMEOUT_S).  ``attempt`` (default: RANGE_DIST_ATTEMPT, else none): a job whose rank
    processes are started a second time against the SAME store (tools/rank_guard.py: fresh children
    after a failed first contact; under torchrun the store lives in the agent and survives them)
    rendezvouses under a prefix of its own, so that nothing the first attempt left in the store -
    rank addresses, RCCL's unique id - is read by the second."""
    from datetime import timedelta

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29500")
    if attempt is None and os.environ.get("RANGE_DIST_ATTEMPT"):
        attempt = int(os.environ["RANGE_DIST_ATTEMPT"])
    if not dist.is_initialized():
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        timeout = timedelta(seconds=dist_timeout_s(timeout_s))
        kw = dict(rank=rank, world_size=world, timeout=timeout)
        if attempt is not None and attempt > 1:
            store, _, _ = next(dist.rendezvous("env://", rank=rank, world_size=world, timeout=timeout))
            store.set_timeout(timeout)
            kw["store"] = dist.PrefixStore(f"range_attempt{attempt}", store)
        if backend == "nccl":
            torch.cuda.set_device(local)
            kw["device_id"] = torch.device("cuda", local)
        dist.init_process_group(backend, **kw)
    return rank, local, world
