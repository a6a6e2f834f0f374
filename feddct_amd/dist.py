"""Aggregation across the GPUs of one node (SURVEY.md §8 e) over
torch.distributed (backend "nccl" = RCCL over xGMI), one process per GPU.
Rank r holds a contiguous shard of the client slots, in slot order
(``shard_range``).

THE DEFAULT ENTRY IS ``Aggregator`` (r05), and it is EXACT: its result is
bit-identical to one GPU reducing every slot, i.e. to the reference's
single-process ``stack(...).mean(0)`` (train_feddct.py:42-50).  Over RCCL it
runs the native library's default round (comm.NativeAggregator: the exact
form — blocked, chained or striped — with the lowest modelled time,
``exact_form``; r06); over any other transport (gloo rehearsals) the chained
or striped round orchestrated here, whichever the model prefers (the blocked
round exists natively only).  The round forms:

* ``ChainAggregator`` (exact client shards): the shards stay put and the
  cascade's accumulator state travels rank to rank in slot order, chunk by
  chunk (fa_reduce_chain); the scalar columns are all-gathered raw.
  Bit-identical;
* ``StripedAggregator`` (e2, exact column stripes): every client's values
  for rank r's column stripe go to rank r, which reduces the stripe over all
  clients; per column chunk ONE batch with every peer (r06).  Bit-identical,
  weighted too;
* ``ShardedAggregator`` (e1, OPT-IN: ``Aggregator(exact=False)``): the HIP
  kernel sums the rank's clients in the torch order without the /N
  (FA_F_SUM_ONLY), chunk by column chunk; each chunk's partial bucket is
  summed across ranks by an RCCL reduce to the server rank (``final=
  "reduce"``) or an all-reduce (``"allreduce"``) while the kernel sums the
  next chunk; then ``/ N_total``.  The cross-rank sum re-associates fp32:
  NOT within the north_star's 1 ULP — measured r04 (2 ranks x 20 wrn16_8
  clients) max 22,938 ULP, histogram in comm.E1_ULP_R04; bench.py's N>1
  line reports it beside the time.

On a native 16-bit layout (``BucketLayout(native16=True)``) the striped round
is the default form: it runs on the fp16 / bf16 buckets themselves, unweighted
(DESIGN §4.14); ``Aggregator`` takes it, the other two classes refuse.  The
chained round on 16-bit buckets is opt-in
(``ChainAggregator(native16=True)``, ``Aggregator(chain16=True)``, DESIGN
§4.15): the cascade state travels in fp32 planes, the clients stay 16-bit
(fa_reduce_chain_elem), and it carries weights — the chain multiplies inside
the kernel, so nothing pre-multiplied travels.

int64 keys (a few bytes) always travel raw — an all-gather of every rank's
int64 buckets — and are reduced exactly over all N_total clients.

The striped round's exchanges follow the native schedule
(``stripe_schedule``: per column chunk one batch of sends and receives with
every peer, the finished chunk two steps later; tests/test_schedule.py checks
the two agree op for op).

The arithmetic backends are pluggable so the orchestration is testable on
CPU with gloo (tests/test_dist_gloo.py injects oracle backends); the product
backends are the Hip* classes.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.distributed as dist

from .layout import BucketLayout


def shard_range(n_total: int, world: int, rank: int):
    """Contiguous client-slot shard of ``rank`` (slot order is preserved)."""
    base, rem = divmod(n_total, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_counts(n_total: int, world: int) -> List[int]:
    """Slots per rank under ``shard_range``."""
    return [b - a for a, b in (shard_range(n_total, world, r) for r in range(world))]


def check_final(final: str) -> None:
    if final not in ("reduce", "allreduce"):
        raise ValueError(f"final must be 'reduce' or 'allreduce', not {final!r}")


def cascade_lp(n: int) -> int:
    """torch's cascade level step for n rows (16 below 2**16 rows)."""
    return max(4, (int(n - 1).bit_length() if n > 1 else 0) // 4)


def blocked_allowed(counts: Sequence[int]) -> bool:
    """The blocked round's precondition (sched_host.cpp first_wide_block): every
    cascade block of 2**lp slots lies on at most two of the ranks holding
    slots."""
    first, n = [], 0
    for c in counts:
        first.append(n)
        n += max(0, int(c))
    q = 1 << cascade_lp(n)
    for a in range(0, n, q):
        b = min(n, a + q)
        on = sum(1 for r, c in enumerate(counts) if c > 0 and first[r] < b and first[r] + c > a)
        if on > 2:
            return False
    return True


def exact_form(counts: Sequence[int], layout: Optional[BucketLayout] = None,
               root_all: bool = False, chain16: bool = False) -> str:
    """The exact round the default entry takes for these shard counts: the
    form with the lowest modelled time (sched_host.cpp fa_multi_select_layout
    on ``layout``; None: fa_multi_select's nominal layout) — "blocked" (only
    where ``blocked_allowed``), "chained" or "striped".  ``root_all``: the
    result goes to every rank.  r05: "blocked" if allowed, else "chained".
    A native 16-bit layout: "striped" (the other forms move fp32 sums or
    cascade state), unless ``chain16`` admits the chained round on 16-bit
    buckets: then the model's pick of the two (fa_multi_select_layout_elem)."""
    from .comm import multi_select
    if layout is not None and layout.native16:
        if not chain16:
            return "striped"   # the one exact form on fp16 / bf16 buckets by default
        return multi_select(counts, layout=layout, root_all=root_all, chain16=True)
    return multi_select(counts, layout=layout, root_all=root_all)


def stripe_schedule(bounds, shards, me, root=-1):
    """The striped round's exchange steps for rank ``me`` (sched_host.cpp
    sched_striped, its steps 2..C+3): per step, in issue order,
    ("send", peer, slot, offset, count) / ("recv", peer, slot, offset, count)
    for client rows, ("send_out", peer, offset, count) / ("recv_out", peer,
    offset, count) for finished chunks, and ("reduce", chunk, offset, count)
    for the stripe reduce that runs beside the step's exchanges.  bounds[r]:
    the C + 1 chunk bounds of rank r's stripe; shards[r]: its slot range."""
    W = len(bounds)
    C = len(bounds[0]) - 1
    result = root < 0 or root == me

    def ln(r, c):
        return bounds[r][c + 1] - bounds[r][c]
    steps = []
    for j in range(C + 2):
        ops = []
        for q in range(1, W):
            r = (me + q) % W
            if j < C:
                if ln(r, j) > 0:
                    ops += [("send", r, k, bounds[r][j], ln(r, j)) for k in range(*shards[me])]
                if ln(me, j) > 0:
                    ops += [("recv", r, k, bounds[me][j], ln(me, j)) for k in range(*shards[r])]
            c = j - 2
            if 0 <= c < C:
                if ln(me, c) > 0 and (root < 0 or root == r):
                    ops.append(("send_out", r, bounds[me][c], ln(me, c)))
                if ln(r, c) > 0 and result:
                    ops.append(("recv_out", r, bounds[r][c], ln(r, c)))
        k = j - 1
        if 0 <= k < C and ln(me, k) > 0:
            ops.append(("reduce", k, bounds[me][k], ln(me, k)))
        steps.append(ops)
    return steps


def p2p(ops, group=None):
    """Post one round of point-to-point ops [(dist.isend | dist.irecv,
    tensor, peer)] together and wait for all of them.  Over gloo (a CPU
    transport, used to rehearse ranks without RCCL) device tensors are staged
    through host copies — gloo would otherwise read device memory from the
    CPU a word at a time; over RCCL the tensors go as they are."""
    if not ops:
        return
    stage = dist.get_backend(group) == "gloo" and any(t.is_cuda for _, t, _ in ops)
    post, back = [], []
    for fn, t, peer in ops:
        if stage and t.is_cuda:
            h = t.cpu() if fn is dist.isend else torch.empty(t.shape, dtype=t.dtype)
            if fn is dist.irecv:
                back.append((t, h))
            t = h
        post.append(dist.P2POp(fn, t, peer, group))
    for req in dist.batch_isend_irecv(post):
        req.wait()
    for t, h in back:
        t.copy_(h)


def refuse_native16(layout: BucketLayout, who: str) -> None:
    """The rounds that exist on fp32 buckets only."""
    if layout.native16:
        raise ValueError(f"{who}: a native {layout.float_dtype} layout runs the striped round "
                         "only (StripedAggregator / Aggregator): this form moves fp32 sums or "
                         "cascade state")


def chunk_segments(layout: BucketLayout, nchunks: int):
    """Split the fp32 segments into <= nchunks consecutive groups of roughly
    equal bytes.  Returns [(segs ndarray, lo, hi)] with [lo, hi) the bucket
    range the group spans (gaps are layout padding)."""
    segs = layout.segs32
    if len(segs) == 0:
        return []
    total = int(segs[:, 1].sum())
    target = max(1, total // max(1, nchunks))
    groups, cur, acc = [], [], 0
    for o, m in segs:
        cur.append((o, m))
        acc += m
        if acc >= target and len(groups) < nchunks - 1:
            groups.append(cur)
            cur, acc = [], 0
    if cur:
        groups.append(cur)
    out = []
    for i, g in enumerate(groups):
        arr = np.array(g, np.int64)
        lo = int(arr[0, 0])
        hi = int(groups[i + 1][0][0]) if i + 1 < len(groups) else layout.f32_numel
        out.append((arr, lo, hi))
    return out


class _HipI64:
    """What the Hip* backends share: the current stream, and the exact int64
    reduce over ``self.plan64`` (None: nothing to reduce)."""

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def reduce_i64(self, clients64: Sequence[torch.Tensor], out64: torch.Tensor):
        if self.plan64 is None:
            return
        L = self._lib
        a = L.ptr_array([t.data_ptr() for t in clients64])
        L.check(L.lib.fa_reduce(self.plan64.handle, None, a, len(clients64), None, None,
                                out64.data_ptr(), 0, self._stream()), "fa_reduce(i64)")


class HipBackend(_HipI64):
    """fa_reduce / fa_div_f32 on the current device and stream."""

    def __init__(self, layout: BucketLayout, chunks, n_local: int, n_total: int):
        from . import _lib
        self._lib = _lib
        self.plans = [_lib.Plan(s, layout.f32_numel) for s, _, _ in chunks]
        self.plan64 = (_lib.Plan(np.zeros((0, 2), np.int64), 0, layout.segs64, layout.i64_numel)
                       if layout.i64_numel else None)

    def partial_sum(self, chunk_index, clients32: Sequence[torch.Tensor], out: torch.Tensor):
        L = self._lib
        a = L.ptr_array([t.data_ptr() for t in clients32])
        L.check(L.lib.fa_reduce(self.plans[chunk_index].handle, a, None, len(clients32), None,
                                out.data_ptr(), None, L.FA_F_SUM_ONLY, self._stream()),
                "fa_reduce(partial)")

    def divide(self, x: torch.Tensor, d: float, out: torch.Tensor):
        L = self._lib
        L.check(L.lib.fa_div_f32(x.data_ptr(), float(d), out.data_ptr(), x.numel(),
                                 self._stream()), "fa_div_f32")


class ShardedAggregator:
    """The cross-GPU round over pre-bound buckets (bench.py's N>1 step).

    ``final="reduce"`` (default): the north_star's final RCCL reduce — the
    global state lands on ``root`` (the server), like the single-process
    reference where the global model is one module; ``final="allreduce"``:
    every rank gets it (reduce + the cross-GPU half of the broadcast).

    ``exchange="reduce"``: one reduce / all-reduce per chunk;
    ``"rs_gather"``: a reduce-scatter (each rank sums 1/W of the chunk) then
    a gather to the root / all-gather — the native FA_XCHG_RS_GATHER; the
    chunk's last len % W floats take the plain reduce."""

    def __init__(self, layout: BucketLayout, local32: List[torch.Tensor],
                 local64: List[torch.Tensor], n_total: int, out32: torch.Tensor,
                 out64: torch.Tensor, nchunks: int = 8, backend=None, group=None,
                 final: str = "reduce", root: int = 0, exchange: str = "reduce"):
        check_final(final)
        if exchange not in ("reduce", "rs_gather"):
            raise ValueError(f"exchange must be 'reduce' or 'rs_gather', not {exchange!r}")
        refuse_native16(layout, "ShardedAggregator")
        self.exchange = exchange
        self.final = final
        self.root = root
        self.rank = dist.get_rank(group)
        self.layout = layout
        self.local32, self.local64 = local32, local64
        self.n_total = n_total
        self.out32, self.out64 = out32, out64
        self.group = group
        self.world = dist.get_world_size(group)
        self.chunks = chunk_segments(layout, nchunks)
        self.backend = backend or HipBackend(layout, self.chunks, len(local32), n_total)
        self.partial = torch.zeros_like(out32)
        # rs_gather: this rank's share of each chunk's sum
        self.shares = []
        off = 0
        for _, lo, hi in self.chunks:
            q = (hi - lo) // self.world if exchange == "rs_gather" else 0
            self.shares.append((off, q))
            off += q
        self.share = torch.zeros(max(off, 1), dtype=out32.dtype, device=out32.device)
        # int64 keys: every rank's buckets gathered raw; shards may be uneven,
        # so each rank sends max-shard rows and only the real ones are used
        nmax = -(-n_total // self.world)
        width = max(1, layout.i64_numel)
        self.gather64 = torch.zeros((self.world * nmax, width), dtype=torch.int64,
                                    device=out64.device)
        self.stack64 = torch.zeros((nmax, width), dtype=torch.int64, device=out64.device)
        rows = []
        for r in range(self.world):
            lo, hi = shard_range(n_total, self.world, r)
            rows += [r * nmax + j for j in range(hi - lo)]
        self.rows64 = rows

    def step(self) -> None:
        works = []
        to_root = self.final == "reduce"
        gdst = self.root if self.group is None else dist.get_global_rank(self.group, self.root)
        has_result = not to_root or self.rank == self.root
        W, me = self.world, self.rank
        for c, (_, lo, hi) in enumerate(self.chunks):
            self.backend.partial_sum(c, self.local32, self.partial)
            so, q = self.shares[c]
            if q:
                # reduce-scatter (completed before its gather is queued: a
                # gloo group may run queued collectives on several threads)
                mine = self.share[so:so + q]
                dist.reduce_scatter_tensor(mine, self.partial[lo:lo + W * q],
                                           op=dist.ReduceOp.SUM, group=self.group)
                if to_root:
                    dst = ([self.out32[lo + r * q:lo + (r + 1) * q] for r in range(W)]
                           if has_result else None)
                    works.append(dist.gather(mine, dst, dst=gdst, group=self.group,
                                             async_op=True))
                else:
                    works.append(dist.all_gather_into_tensor(self.out32[lo:lo + W * q], mine,
                                                             group=self.group, async_op=True))
            rlo = lo + W * q
            if rlo < hi:
                if to_root:
                    works.append(dist.reduce(self.partial[rlo:hi], dst=gdst,
                                             op=dist.ReduceOp.SUM, group=self.group,
                                             async_op=True))
                else:
                    works.append(dist.all_reduce(self.partial[rlo:hi], op=dist.ReduceOp.SUM,
                                                 group=self.group, async_op=True))
            works.append(None)   # chunk boundary
        w64 = None
        if self.layout.i64_numel:
            for j, t in enumerate(self.local64):
                self.stack64[j].copy_(t)
            w64 = dist.all_gather_into_tensor(self.gather64, self.stack64, group=self.group,
                                              async_op=True)
        # finish chunk c (/N_total) as soon as its exchange lands, while the
        # exchanges of the later chunks are still on the wire
        c = 0
        for w in works:
            if w is not None:
                w.wait()
                continue
            _, lo, hi = self.chunks[c]
            so, q = self.shares[c]
            if has_result:
                if q == 0:      # the reduced chunk sits in partial (root / all-reduce)
                    self.backend.divide(self.partial[lo:hi], float(self.n_total),
                                        self.out32[lo:hi])
                else:           # shares gathered into out32; the remainder in partial
                    rlo = lo + W * q
                    if rlo < hi:
                        self.out32[rlo:hi].copy_(self.partial[rlo:hi])
                    self.backend.divide(self.out32[lo:hi], float(self.n_total),
                                        self.out32[lo:hi])
            c += 1
        if w64 is not None:
            w64.wait()
            if has_result:
                self.backend.reduce_i64([self.gather64[r] for r in self.rows64], self.out64)


# --------------------------------------------------------------------------
# Exact mode: element (column) stripes.
# --------------------------------------------------------------------------
class HipStripeBackend(_HipI64):
    """Stripe-chunk reductions with the HIP kernel over tile-subset plans
    (one per chunk of this rank's stripe).  ``elem``: the floating bucket's
    element type (default: the layout's — FA_ELEM_F16 / FA_ELEM_BF16 on a
    native 16-bit layout, whose chunk plans are 16-bit ones)."""

    def __init__(self, layout: BucketLayout, chunk_tiles, tiles64, elem=None):
        from . import _lib
        from .partition import layout_elem
        self._lib = _lib
        te = 0
        if elem is None:
            elem = layout_elem(layout)
        self.elem = _lib.FA_ELEM_F32 if elem is None else int(elem)
        self.esize = 4 if self.elem == _lib.FA_ELEM_F32 else 2
        if self.elem == _lib.FA_ELEM_F32:
            self.plans = [_lib.Plan(None, layout.f32_numel, None, layout.i64_numel, te, tiles=t)
                          if len(t) else None for t in chunk_tiles]
        else:
            self.plans = [_lib.Plan.from_tiles(t, layout.f32_numel, layout.i64_numel, te,
                                               _lib.FA_PLAN_GAPS_ARE_PADDING, self.elem)
                          if len(t) else None for t in chunk_tiles]
        self.plan64 = (_lib.Plan(None, layout.f32_numel, None, layout.i64_numel, te,
                                 tiles=tiles64) if len(tiles64) else None)

    def reduce_chunk(self, c, lo, hi, sources, out32: torch.Tensor, weights=None):
        """Chunk ``c`` ([lo, hi)) over every client: ``sources[k] = (tensor,
        base)``, client slot k's element e at ``tensor[e - base]``; weights:
        None (the mean) or n_total fp32 weights (no division)."""
        if self.plans[c] is None:
            return
        L = self._lib
        if weights is not None and self.esize != 4:
            raise ValueError("HipStripeBackend: weighted rounds on 16-bit buckets are not built")
        ptrs = [t.data_ptr() - self.esize * base for t, base in sources]
        w = None if weights is None else (ctypes.c_float * len(weights))(*map(float, weights))
        L.check(L.lib.fa_reduce(self.plans[c].handle, L.ptr_array(ptrs), None, len(ptrs), w,
                                out32.data_ptr(), None, 0, self._stream()),
                "fa_reduce(stripe chunk)")


class StripedAggregator:
    """Bit-exact cross-GPU round: rank r owns the column stripe
    [lo_r, hi_r) of the bucket (cut at vector-tile starts, partition.py), cut
    into ``nchunks`` column chunks; it gets every client's values for those
    columns, reduces them in the exact torch order and the finished chunks
    go to the result ranks (every rank: ``final="allreduce"``; ``root``:
    ``"reduce"``).  Two ingress forms:

    * ``step_device(local32, local64, weights=None)`` — client slots
      device-resident and sharded by rank (``counts``, default shard_range):
      per chunk ONE batch of sends and receives with every peer (r06: the
      native schedule, ``stripe_schedule``; r02-r05 one partner at a time),
      n·B·(W-1)/W per rank over the round.  Weighted: the rows a rank sends
      are its clients' values pre-multiplied by their weights (rounded as the
      weighted kernel rounds the product), the receiver reduces them with
      weight 1;
    * ``step_host(stripes32, clients64)`` — client updates in host memory:
      each GPU uploads only ITS stripe of every client (no xGMI traffic for
      inputs; ingress bandwidth scales with the GPUs' PCIe links).

    The result is the same bits as the single-GPU reduction (tested).  Only
    the result ranks' ``out32`` / ``out64`` are written, the int64 keys too.
    """

    def __init__(self, layout: BucketLayout, n_total: int, out32: torch.Tensor,
                 out64: torch.Tensor, group=None, backend=None, final: str = "allreduce",
                 root: int = 0, nchunks: int = 4, counts: Optional[Sequence[int]] = None):
        from .partition import cut_align, i64_tiles, layout_tiles, stripe_chunks
        check_final(final)
        if layout.native16 and out32.dtype != layout.float_dtype:
            raise TypeError(f"StripedAggregator: a {out32.dtype} result bucket on a "
                            f"{layout.float_dtype} layout")
        self.final = final
        self.root = root if final == "reduce" else -1
        self.layout = layout
        self.n_total = n_total
        self.out32, self.out64 = out32, out64
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        if counts is None:
            counts = shard_counts(n_total, self.world)
        self.counts = [int(c) for c in counts]
        if len(self.counts) != self.world or sum(self.counts) != n_total:
            raise ValueError(f"counts {self.counts} do not shard {n_total} slots over "
                             f"{self.world} ranks")
        first = [sum(self.counts[:r]) for r in range(self.world)]
        self.shards = [(first[r], first[r] + self.counts[r]) for r in range(self.world)]
        info, tiles = layout_tiles(layout)
        self.chunks = stripe_chunks(tiles, self.world, layout.f32_numel, nchunks,
                                    cut_align(layout))
        self.bounds = [[c[0] for c in ch] + [ch[-1][1]] for ch in self.chunks]
        self.ranges = [(b[0], b[-1]) for b in self.bounds]
        self.lo, self.hi = self.ranges[self.rank]
        self.backend = backend or HipStripeBackend(layout, [t for _, _, t in self.chunks[self.rank]],
                                                   i64_tiles(tiles))
        L = self.hi - self.lo
        # rows stay 16-B aligned: 4 floats, 8 elements of a 16-bit layout
        q = 8 if layout.native16 else 4
        self.lpad = (L + q - 1) // q * q
        dev = out32.device
        self.recv = torch.zeros((n_total, max(self.lpad, q)), dtype=layout.float_dtype, device=dev)
        self.stage = None   # weighted rounds: pre-multiplied local clients
        nmax = max(1, max(self.counts))
        width = max(1, layout.i64_numel)
        self.gather64 = torch.zeros((self.world * nmax, width), dtype=torch.int64, device=dev)
        self.stack64 = torch.zeros((nmax, width), dtype=torch.int64, device=dev)
        self.rows64 = [r * nmax + j for r in range(self.world) for j in range(self.counts[r])]

    def _peer(self, r):
        return r if self.group is None else dist.get_global_rank(self.group, r)

    def _i64(self, local64):
        if not self.layout.i64_numel:
            return
        for j, t in enumerate(local64):
            self.stack64[j].copy_(t)
        dist.all_gather_into_tensor(self.gather64, self.stack64, group=self.group)
        if self.root < 0 or self.root == self.rank:   # out64 belongs to the result ranks
            self.backend.reduce_i64([self.gather64[r] for r in self.rows64], self.out64)

    def schedule(self):
        """This rank's exchange steps, in issue order (``stripe_schedule``)."""
        return stripe_schedule(self.bounds, self.shards, self.rank, self.root)

    def _dst(self):
        result = self.root < 0 or self.root == self.rank
        return self.out32 if result else self.out32.new_empty(self.out32.shape)

    def step_device(self, local32: List[torch.Tensor], local64: List[torch.Tensor],
                    weights: Optional[Sequence[float]] = None) -> None:
        me = self.rank
        a, b = self.shards[me]
        if len(local32) != b - a:
            raise ValueError(f"rank {me} holds {len(local32)} clients, shard is {b - a}")
        self._check16(local32, weights)
        self._i64(local64)
        send = local32
        wfull = None
        if weights is not None:
            if len(weights) != b - a:
                raise ValueError(f"{len(weights)} weights for {b - a} clients")
            send = []
            for j, t in enumerate(local32):
                # (a Python scalar: a device tensor made from one is a blocking
                # upload, a stream synchronisation per client)
                send.append(t * float(np.float32(weights[j])))
            wfull = [1.0] * self.n_total
            for j in range(b - a):
                wfull[a + j] = float(np.float32(weights[j]))
        sources = [(local32[k - a], 0) if a <= k < b else (self.recv[k], self.lo)
                   for k in range(self.n_total)]
        dst = self._dst()
        for ops in self.schedule():
            post, red = [], None
            for op in ops:
                kind = op[0]
                if kind == "send":
                    _, r, slot, off, cnt = op
                    post.append((dist.isend, send[slot - a][off:off + cnt], self._peer(r)))
                elif kind == "recv":
                    _, r, slot, off, cnt = op
                    post.append((dist.irecv, self.recv[slot, off - self.lo:off - self.lo + cnt],
                                 self._peer(r)))
                elif kind == "send_out":
                    _, r, off, cnt = op
                    post.append((dist.isend, dst[off:off + cnt], self._peer(r)))
                elif kind == "recv_out":
                    _, r, off, cnt = op
                    post.append((dist.irecv, self.out32[off:off + cnt], self._peer(r)))
                else:
                    red = op
            p2p(post, self.group)
            if red is not None:
                _, c, off, cnt = red
                self.backend.reduce_chunk(c, off, off + cnt, sources, dst, wfull)

    def _check16(self, tensors, weights=None):
        """A native 16-bit layout's round: buckets of the layout's dtype, no
        weights — checked before any exchange, so every rank refuses alike."""
        if not self.layout.native16:
            return
        if weights is not None:
            raise ValueError("StripedAggregator: weighted rounds on 16-bit buckets are not built "
                             "(the pre-multiplied rows are fp32 values)")
        for t in tensors:
            if t.dtype != self.layout.float_dtype:
                raise TypeError(f"StripedAggregator: a {t.dtype} bucket on a native "
                                f"{self.layout.float_dtype} layout")

    def step_host(self, stripes32: Sequence[torch.Tensor], clients64: Sequence[torch.Tensor],
                  local64: Optional[List[torch.Tensor]] = None) -> None:
        """``stripes32[k]``: client slot k's values for THIS rank's columns
        [lo, hi) (host, pinned; the layout's dtype), ``clients64[k]``: its
        int64 bucket."""
        self._check16(stripes32)
        L = self.hi - self.lo
        for k, t in enumerate(stripes32):
            self.recv[k, :L].copy_(t, non_blocking=True)
        dst = self._dst()
        sources = [(self.recv[k], self.lo) for k in range(self.n_total)]
        for c, (lo, hi, _) in enumerate(self.chunks[self.rank]):
            if hi > lo:
                self.backend.reduce_chunk(c, lo, hi, sources, dst)
        me, result = self.rank, self.root < 0 or self.root == self.rank
        if self.layout.i64_numel and result:   # out64 belongs to the result ranks
            g = torch.stack([t.to(self.out64.device, non_blocking=True) for t in clients64])
            self.backend.reduce_i64(list(g.unbind(0)), self.out64)
        # the finished stripes to the result ranks, every peer in one batch
        post = []
        for q in range(1, self.world):
            r = (me + q) % self.world
            lo, hi = self.ranges[r]
            if self.hi > self.lo and (self.root < 0 or self.root == r):
                post.append((dist.isend, dst[self.lo:self.hi], self._peer(r)))
            if hi > lo and result:
                post.append((dist.irecv, self.out32[lo:hi], self._peer(r)))
        p2p(post, self.group)


# --------------------------------------------------------------------------
# Exact client shards: the cascade state travels (fa_reduce_chain).
# --------------------------------------------------------------------------
def chain_levels(rows: int, n_total: int) -> int:
    """Bit l: state plane l may be nonzero after ``rows`` of ``n_total`` rows
    (fa_chain_levels; the cascade's level step is 16 below 2**16 clients)."""
    if rows <= 0:
        return 0
    lp = max(4, (int(n_total - 1).bit_length() if n_total > 1 else 0) // 4)
    step = 1 << lp
    m = 0
    if rows % step:
        m |= 1
    if (rows >> lp) % step:
        m |= 2
    if n_total >= 256:
        if (rows >> (2 * lp)) % step:
            m |= 4
        if rows >> (3 * lp):
            m |= 8
    return m


class HipChainBackend(_HipI64):
    """fa_reduce_chain_elem over the vector-tile chunks; the raw scalar columns
    (compact tail plan + int64 plan) reduced with fa_reduce.  ``elem``: the
    floating bucket's element type (default: the layout's — FA_ELEM_F16 /
    FA_ELEM_BF16 on a native 16-bit layout: 16-bit chunk plans, a 16-bit
    compact tail plan, fp32 state planes)."""

    def __init__(self, layout: BucketLayout, chunks, compact, tidx, t64, elem=None):
        from . import _lib
        from .partition import layout_elem
        self._lib = _lib
        self.layout = layout
        if elem is None:
            elem = layout_elem(layout)
        self.elem = _lib.FA_ELEM_F32 if elem is None else int(elem)
        pad = _lib.FA_PLAN_GAPS_ARE_PADDING
        self.plans = [_lib.Plan.from_tiles(t, layout.f32_numel, 0, 0, pad, self.elem)
                      for _, _, t in chunks]
        T = len(tidx)
        self.plan_t32 = _lib.Plan.from_tiles(compact, T, 0, 0, pad, self.elem) if T else None
        self.plan64 = (_lib.Plan(None, layout.f32_numel, None, layout.i64_numel, 0, tiles=t64)
                       if len(t64) else None)
        self.tout = None

    def chain(self, c, clients32, row0, n_total, state, state_in, out, plane, weights=None):
        L = self._lib
        ch = L.FaChain(row0, n_total, state.data_ptr() if state_in else None,
                       None if out is not None else state.data_ptr(), plane)
        w = None if weights is None else (ctypes.c_float * len(weights))(*map(float, weights))
        L.check(L.lib.fa_reduce_chain_elem(self.plans[c].handle,
                                           L.ptr_array([t.data_ptr() for t in clients32]),
                                           len(clients32), w, ctypes.byref(ch),
                                           out.data_ptr() if out is not None else None, 0,
                                           self._stream()), "fa_reduce_chain_elem")

    def tails(self, rows32, tidx, out32, weighted, weights=None):
        """The gathered scalar columns into ``out32[tidx]``.  fp32 rows of a
        weighted round arrive pre-multiplied (the ordered sum, no division);
        16-bit rows arrive raw and ``weights`` holds every row's weight (a
        16-bit plan has no FA_F_SUM_ONLY: the weighted reduce itself)."""
        L = self._lib
        if self.tout is None:
            self.tout = torch.zeros(max(64, -(-len(tidx) // 64) * 64), dtype=out32.dtype,
                                    device=out32.device)
        w = None if weights is None else (ctypes.c_float * len(weights))(*map(float, weights))
        flags = L.FA_F_SUM_ONLY if weighted and weights is None else 0
        L.check(L.lib.fa_reduce(self.plan_t32.handle, L.ptr_array([r.data_ptr() for r in rows32]),
                                None, len(rows32), w, self.tout.data_ptr(), None, flags,
                                self._stream()), "fa_reduce(tails)")
        out32[tidx] = self.tout[:len(tidx)]


class ChainAggregator:
    """Exact client-sharded round over torch.distributed (the Python form of
    the native fa_reduce_chained; same cut, same hops, same tails).

    Rank r holds slots ``shards[r]`` (contiguous, slot order).  Per vector
    column chunk, rank r receives the cascade state after slots
    0..first[r]-1 from rank r-1, continues it over its own clients
    (fa_reduce_chain) and sends it on to rank r+1; the last rank holding
    clients finishes the mean.  Only the state planes chain_levels() names
    travel — one float per element below 16 slots, two below 256.  The
    scalar columns (ILP-4 tails, M==1) and int64 keys are all-gathered raw and
    reduced by the result ranks.  ``final="reduce"``: the result on ``root``;
    ``"allreduce"``: on every rank (a broadcast from the finisher).

    ``native16=True`` admits a native 16-bit layout (refused otherwise): the
    clients, the result, the stacked scalar columns and the finisher's buffer
    are fp16 / bf16, the state planes stay fp32 and travel as on fp32 buckets.
    Weighted, the chain multiplies by the local weights inside the kernel, the
    scalar columns are gathered raw and the ranks' weights beside them, and the
    result ranks run the weighted reduce over the gathered rows."""

    def __init__(self, layout: BucketLayout, n_total: int, out32: torch.Tensor,
                 out64: torch.Tensor, group=None, backend=None, final: str = "reduce",
                 root: int = 0, nchunks: int = 16, counts: Optional[Sequence[int]] = None,
                 native16: bool = False):
        from .partition import chain_cut
        check_final(final)
        if not native16:
            refuse_native16(layout, "ChainAggregator")
        if layout.native16 and out32.dtype != layout.float_dtype:
            raise TypeError(f"ChainAggregator: a {out32.dtype} result bucket on a "
                            f"{layout.float_dtype} layout")
        self.layout, self.n_total = layout, n_total
        self.out32, self.out64 = out32, out64
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.root = root if final == "reduce" else -1
        if counts is None:
            counts = shard_counts(n_total, self.world)
        self.counts = list(counts)
        self.first = [sum(self.counts[:r]) for r in range(self.world)]
        self.finisher = max(r for r in range(self.world) if self.counts[r] > 0)
        self.chunks, compact, tidx, t64 = chain_cut(layout, nchunks)
        dev = out32.device
        self.tidx = torch.from_numpy(tidx).to(dev)
        self.T = len(tidx)
        self.trow = -(-self.T // 64) * 64
        self.backend = backend or HipChainBackend(layout, self.chunks, compact, tidx, t64)
        self.plane = -(-layout.f32_numel // 64) * 64
        nplanes = 4 if n_total >= 256 else 2
        self.state = torch.zeros(nplanes * self.plane, dtype=torch.float32, device=dev)
        me = self.rank
        self.lev_in = chain_levels(self.first[me], n_total)
        self.lev_out = chain_levels(self.first[me] + self.counts[me], n_total)
        self.fin = (torch.zeros_like(out32) if me == self.finisher and self.root >= 0
                    and self.root != me else None)
        nmax = max(self.counts)
        self.nmax = nmax
        # (the layout's dtype: fp32, or the raw 16-bit rows of a native 16-bit layout)
        self.stack32 = torch.zeros((nmax, max(self.trow, 1)), dtype=layout.float_dtype, device=dev)
        self.gather32 = torch.zeros((self.world * nmax, max(self.trow, 1)),
                                    dtype=layout.float_dtype, device=dev)
        # a weighted 16-bit round: the ranks' weights, padded to nmax
        self.wstack = torch.zeros(nmax, dtype=torch.float32, device=dev)
        self.wgather = torch.zeros(self.world * nmax, dtype=torch.float32, device=dev)
        w64 = max(1, layout.i64_numel)
        self.stack64 = torch.zeros((nmax, w64), dtype=torch.int64, device=dev)
        self.gather64 = torch.zeros((self.world * nmax, w64), dtype=torch.int64, device=dev)
        self.rows = [r * nmax + j for r in range(self.world) for j in range(self.counts[r])]

    def _peer(self, r):
        return r if self.group is None else dist.get_global_rank(self.group, r)

    def _planes(self, lev, lo, hi):
        return [self.state[l * self.plane + lo:l * self.plane + hi] for l in range(4)
                if lev & (1 << l)]

    def step(self, local32: List[torch.Tensor], local64: List[torch.Tensor],
             weights: Optional[Sequence[float]] = None) -> None:
        me, F = self.rank, self.finisher
        n_loc = self.counts[me]
        assert len(local32) == n_loc
        h16 = self.layout.native16
        for t in local32:   # before any exchange, so every rank refuses alike
            if h16 and t.dtype != self.layout.float_dtype:
                raise TypeError(f"ChainAggregator: a {t.dtype} bucket on a native "
                                f"{self.layout.float_dtype} layout")
        result = self.root < 0 or self.root == me
        # the raw scalar columns: stacked, gathered while the chain runs
        if self.T:
            for j, t in enumerate(local32):
                v = t[self.tidx]
                if weights is not None and not h16:
                    # a Python scalar, not a device tensor made from one: that
                    # is a blocking upload, one stream synchronisation per client
                    # (the product is the same fp32 multiply by the fp32 weight)
                    v = v * float(np.float32(weights[j]))
                self.stack32[j, :self.T] = v
        for j, t in enumerate(local64):
            self.stack64[j].copy_(t)
        gw = []
        if self.T:
            gw.append(dist.all_gather_into_tensor(self.gather32, self.stack32, group=self.group,
                                                  async_op=True))
        if self.layout.i64_numel:
            gw.append(dist.all_gather_into_tensor(self.gather64, self.stack64, group=self.group,
                                                  async_op=True))
        wgather = h16 and weights is not None and self.T
        if wgather:   # 16-bit rows travel raw: the result ranks need every weight
            self.wstack.zero_()
            if n_loc:
                self.wstack[:n_loc] = torch.from_numpy(np.asarray(weights, np.float32))
            gw.append(dist.all_gather_into_tensor(self.wgather, self.wstack, group=self.group,
                                                  async_op=True))
        for w in gw:   # (gloo runs collectives and P2P on one thread: finish first)
            w.wait()
        # the chain
        sends = []
        if me <= F:
            pred = me > 0 and self.lev_in
            succ = me < F and self.lev_out
            dst = None if me < F else (self.out32 if result else self.fin)
            staged = dist.get_backend(self.group) == "gloo" and self.state.is_cuda
            for c, (lo, hi, _) in enumerate(self.chunks):
                if pred:
                    p2p([(dist.irecv, p, self._peer(me - 1))
                         for p in self._planes(self.lev_in, lo, hi)], self.group)
                if n_loc:
                    self.backend.chain(c, local32, self.first[me], self.n_total, self.state,
                                       bool(pred), dst, self.plane, weights)
                if succ:
                    planes = self._planes(self.lev_out, lo, hi)
                    if staged:     # (gloo rehearsal: host copies, see p2p)
                        planes = [p.cpu() for p in planes]
                    sends += dist.batch_isend_irecv(
                        [dist.P2POp(dist.isend, p, self._peer(me + 1), self.group)
                         for p in planes])
        for req in sends:
            req.wait()
        if self.chunks:
            lo, hi = self.chunks[0][0], self.chunks[-1][1]
            if self.root < 0:
                dist.broadcast(self.out32[lo:hi], src=self._peer(F), group=self.group)
            elif self.root != F:
                if me == F:
                    p2p([(dist.isend, self.fin[lo:hi], self._peer(self.root))], self.group)
                elif me == self.root:
                    p2p([(dist.irecv, self.out32[lo:hi], self._peer(F))], self.group)
        if result:
            if self.T:
                wall = self.wgather.cpu().numpy()[self.rows] if wgather else None
                self.backend.tails([self.gather32[r] for r in self.rows], self.tidx, self.out32,
                                   weights is not None, *(() if wall is None else (wall,)))
            self.backend.reduce_i64([self.gather64[r] for r in self.rows], self.out64)


# --------------------------------------------------------------------------
# The default entry (r05): exact.
# --------------------------------------------------------------------------
class Aggregator:
    """THE multi-GPU round (SURVEY.md §8 e; BASELINE config 5): this rank's
    client slots ``local32`` / ``local64`` (a contiguous shard, slot order)
    reduced with every other rank's into ``out32`` / ``out64``.

    ``exact=True`` (default): bit-identical to one GPU reducing all
    ``n_total`` slots (the reference's train_feddct.py:42-50 order).  Over an
    RCCL ("nccl") group the native library's default round
    (comm.NativeAggregator: the form and chunk count the cost model picks,
    ``exact_form(counts, layout)``, ONE C call per round on the library's own
    communicator); over any other backend, or with injected arithmetic
    backends (tests: ``backend`` for the chained form, ``stripe_backend`` for
    the striped one), the round orchestrated over torch.distributed — the
    striped form (``StripedAggregator``) where the model picks it, else the
    chained one (``ChainAggregator``; the blocked round exists natively
    only).

    ``exact=False``: the re-associated e1 round (``ShardedAggregator``):
    unweighted only; NOT within 1 ULP (max 22,938 ULP measured r04,
    comm.E1_ULP_R04).

    ``final="reduce"`` puts the result on ``root`` (default: the last rank
    holding slots, where the chained round ends); ``"allreduce"`` on every
    rank.  ``weights``: this rank's fp32 client weights (exact rounds only).
    ``self.form`` names what runs, e.g. "blocked/native".

    ``chain16=True`` (a native 16-bit layout): the chained round on 16-bit
    buckets joins the candidates — the form ``exact_form(..., chain16=True)``
    picks, and with ``weights`` the chained form (the striped 16-bit round
    still refuses weights)."""

    def __init__(self, layout: BucketLayout, local32: List[torch.Tensor],
                 local64: List[torch.Tensor], n_total: int, out32: torch.Tensor,
                 out64: torch.Tensor, group=None, final: str = "reduce",
                 root: Optional[int] = None, weights: Optional[Sequence[float]] = None,
                 counts: Optional[Sequence[int]] = None, exact: bool = True,
                 native: Optional[bool] = None, backend=None, nchunks: Optional[int] = None,
                 stripe_backend=None, chain16: bool = False):
        check_final(final)
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        if counts is None:
            counts = shard_counts(n_total, world)
        counts = [int(c) for c in counts]
        if len(counts) != world or sum(counts) != n_total or len(local32) != counts[rank]:
            raise ValueError(f"rank {rank} holds {len(local32)} clients; counts {counts} "
                             f"over {world} ranks must sum to {n_total}")
        if root is None:
            root = max(r for r in range(world) if counts[r] > 0)
        self.local32, self.local64, self.weights = local32, local64, weights
        self.counts = counts
        if not exact:
            if weights is not None:
                raise ValueError("the re-associated e1 round is unweighted")
            if counts != shard_counts(n_total, world):
                raise ValueError("the e1 round takes shard_range shards")
            self._agg = ShardedAggregator(layout, local32, local64, n_total, out32, out64,
                                          nchunks=nchunks or 8, backend=backend, group=group,
                                          final=final, root=root)
            self.form = "e1/torch.distributed"
            self._step = self._agg.step
            return
        chain16 = bool(chain16) and layout.native16
        if layout.native16 and exact and weights is not None and not chain16:
            raise ValueError("Aggregator: weighted rounds on 16-bit buckets are not built (the "
                             "pre-multiplied rows are fp32 values)")

        def form():
            if chain16 and weights is not None:
                return "chained"   # the one 16-bit round that carries weights
            return exact_form(counts, layout, root_all=final != "reduce", chain16=chain16)
        if layout.native16 and backend is not None and stripe_backend is None \
                and not (chain16 and form() == "chained"):
            # (the fp32 path keeps its behaviour: there the model may still pick
            # the chained form, which ``backend`` serves)
            raise ValueError("Aggregator: a native 16-bit layout runs the striped round, whose "
                             "arithmetic backend is `stripe_backend`; `backend` (the chained "
                             "form's) alone would silently mix in HipStripeBackend")
        if native is None:
            # (the native rounds run on fp32 buckets only)
            native = (backend is None and stripe_backend is None and not layout.native16
                      and "nccl" in str(dist.get_backend(group)))
        if native:
            from .comm import Comm, NativeAggregator
            self._comm = Comm.from_process_group(group)
            self._agg = NativeAggregator(layout, local32, local64, n_total, out32, out64,
                                         self._comm, final=final, root=root, weights=weights,
                                         counts=counts, nchunks=nchunks or 0)
            self.form = f"{self._agg.mode}/native"
            self._step = self._agg.step
        elif form() == "striped":
            self._agg = StripedAggregator(layout, n_total, out32, out64, group=group,
                                          backend=stripe_backend, final=final, root=root,
                                          nchunks=nchunks or 4, counts=counts)
            self.form = "striped/torch.distributed"
            self._step = lambda: self._agg.step_device(self.local32, self.local64, self.weights)
        else:
            self._agg = ChainAggregator(layout, n_total, out32, out64, group=group,
                                        backend=backend, final=final, root=root,
                                        nchunks=nchunks or 16, counts=counts, native16=chain16)
            self.form = "chained/torch.distributed"
            self._step = lambda: self._agg.step(self.local32, self.local64, self.weights)

    def step(self) -> None:
        """One round, stream-ordered on the current stream."""
        self._step()
