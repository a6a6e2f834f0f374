"""An in-process stand-in for ``torch.distributed`` (test infrastructure
only): W ranks as W Python threads of the test process, so that
feddct_amd/dist.py's rounds run with their real arithmetic backends at more
than one rank on ONE device (RCCL refuses two ranks on a device; a gloo
rehearsal needs one GPU process per rank).

Use::

    loop = LoopDist(world)
    monkeypatch.setattr(feddct_amd.dist, "dist", loop)
    results = run_ranks(world, fn)          # fn(rank) in W threads

It implements exactly what dist.py uses, with torch.distributed's meaning:
get_world_size / get_rank (per thread) / get_global_rank / get_backend,
isend / irecv / P2POp / batch_isend_irecv, all_gather_into_tensor, broadcast,
reduce, all_reduce, reduce_scatter_tensor, gather (``async_op=True`` returns
a waitable), ReduceOp.SUM and barrier.  No process is started and no process
group is created.

Rules:

* ``get_backend`` answers "loop": neither "gloo" (dist.py's host staging is
  not taken) nor an "nccl" name (the native round is not taken).
* A send clones its tensor and synchronises the sender's current stream
  before the payload is handed over; the receiver copies it into the
  destination on its own current stream.  Device tensors stay on the device.
* Point-to-point messages match per (source, destination) pair in posting
  order: the k-th irecv posted for a pair takes the pair's k-th isend,
  whatever the order of the ``wait()`` calls.  A payload whose size or dtype
  differs from the posted receive raises (real transports would corrupt or
  hang).
* Collectives match in call order (every rank must call the same collective
  next; a mismatch raises).
* ``ReduceOp.SUM`` ADDS THE RANKS' CONTRIBUTIONS IN ASCENDING RANK ORDER IN
  THE TENSOR'S OWN PRECISION: ``((p0 + p1) + p2) + ...`` — fp32 for the e1
  round's partial buckets.  The e1 expectations of tests/test_distloop_cpu.py
  and tests/test_gpu_dist_loopback.py are built on exactly this order.
  reduce: only ``dst``'s tensor is written.
* Every blocking wait has a time limit (``LoopDist.timeout``, at most 60 s)
  and raises TimeoutError when it runs out.  The first exception in any rank
  sets a shared flag that makes every other rank's next (or current) wait
  raise at once.  ``run_ranks`` joins the daemon rank threads with a limit,
  re-raises the first error and retries nothing: a deadlock ends as a failed
  test, never as a hung run.
* Each rank thread calls ``torch.cuda.set_device`` itself when a device is
  given.  All ranks share the default stream.
* One rank runs at a time: a rank thread holds the harness lock while it
  runs and lets go of it only inside a blocking wait.  The product runs one
  process per rank, so its backends are never entered by two threads at
  once; the harness keeps it so.  The kernels of different ranks still queue
  behind each other on the device like any stream-ordered work.
"""
import threading
import time

import torch

MAX_WAIT_S = 60.0


class LoopError(RuntimeError):
    """Misuse the real transport would answer with a hang or corruption."""


class _Done:
    """A request that needs no waiting (sends: the payload is handed over)."""

    def wait(self):
        return True


class _Pending:
    def __init__(self, finish):
        self._finish, self._done = finish, False

    def wait(self):
        if not self._done:
            self._finish()
            self._done = True
        return True


class ReduceOp:
    SUM = "sum"


class P2POp:
    def __init__(self, op, tensor, peer, group=None, tag=0):
        self.op, self.tensor, self.peer, self.group = op, tensor, peer, group


class LoopDist:
    ReduceOp = ReduceOp
    P2POp = P2POp

    def __init__(self, world: int, timeout: float = 30.0):
        if world < 1:
            raise ValueError("world must be >= 1")
        self.world = world
        self.timeout = min(float(timeout), MAX_WAIT_S)
        self._cond = threading.Condition()      # the harness lock (see module doc)
        self._tls = threading.local()
        self.error = None                       # first exception of any rank
        self._sent = {}                         # (src, dst) -> messages posted
        self._posted = {}                       # (src, dst) -> receives posted
        self._mail = {}                         # (src, dst, seq) -> payload
        self._cseq = [0] * world                # per rank: collectives called
        self._coll = {}                         # seq -> {"op", "parts", "taken"}
        # stable identities: dist.py compares ``fn is dist.isend``
        self.isend, self.irecv = self._isend, self._irecv

    # ------------------------------------------------------------ identity --
    def _bind(self, rank):
        self._tls.rank = rank

    def get_rank(self, group=None):
        try:
            return self._tls.rank
        except AttributeError:
            raise LoopError("get_rank outside a rank thread (run_ranks)") from None

    def get_world_size(self, group=None):
        return self.world

    def get_global_rank(self, group, rank):
        return rank

    def get_backend(self, group=None):
        return "loop"

    # ------------------------------------------------------------- waiting --
    def fail(self, exc):
        """Record the first error; every waiter raises at its next wake-up."""
        if self.error is None:
            self.error = exc

    def _wait_for(self, ready, what):
        """Called with the harness lock held; gives it up while blocked."""
        end = time.monotonic() + self.timeout
        while True:
            if self.error is not None:
                raise LoopError(f"rank {self.get_rank()}: another rank failed while this one "
                                f"waited for {what}: {self.error!r}")
            if ready():
                return
            left = end - time.monotonic()
            if left <= 0:
                raise TimeoutError(f"rank {self.get_rank()}: no {what} within {self.timeout} s")
            self._cond.wait(min(left, 0.25))

    @staticmethod
    def _payload(t):
        p = t.detach().clone()
        if p.is_cuda:
            torch.cuda.current_stream(p.device).synchronize()
        return p

    # ------------------------------------------------------ point to point --
    def _isend(self, tensor, dst, group=None, tag=0):
        me = self.get_rank()
        if not 0 <= dst < self.world or dst == me:
            raise LoopError(f"rank {me}: isend to rank {dst}")
        p = self._payload(tensor)
        with self._cond:
            k = self._sent.get((me, dst), 0)
            self._sent[(me, dst)] = k + 1
            self._mail[(me, dst, k)] = p
            self._cond.notify_all()
        return _Done()

    def _irecv(self, tensor, src, group=None, tag=0):
        me = self.get_rank()
        if not 0 <= src < self.world or src == me:
            raise LoopError(f"rank {me}: irecv from rank {src}")
        with self._cond:
            k = self._posted.get((src, me), 0)
            self._posted[(src, me)] = k + 1
        key = (src, me, k)

        def finish():
            with self._cond:
                self._wait_for(lambda: key in self._mail, f"message {k} from rank {src}")
                p = self._mail.pop(key)
            if p.numel() != tensor.numel() or p.dtype != tensor.dtype:
                raise LoopError(f"rank {me}: message {k} from rank {src} is {p.numel()} x "
                                f"{p.dtype}, the posted receive {tensor.numel()} x {tensor.dtype}")
            tensor.copy_(p.view(tensor.shape))
        return _Pending(finish)

    def batch_isend_irecv(self, ops):
        reqs = []
        for op in ops:
            if op.op is self.isend:
                reqs.append(self._isend(op.tensor, op.peer, op.group))
            elif op.op is self.irecv:
                reqs.append(self._irecv(op.tensor, op.peer, op.group))
            else:
                raise LoopError(f"P2POp of {op.op!r}")
        return reqs

    # --------------------------------------------------------- collectives --
    def _collective(self, op, part, apply, async_op):
        """Deposit this rank's ``part`` for its next collective; ``apply(parts)``
        (parts[r] = rank r's deposit) writes this rank's result once every
        rank has deposited."""
        me = self.get_rank()
        with self._cond:
            seq = self._cseq[me]
            self._cseq[me] += 1
            slot = self._coll.setdefault(seq, {"op": op, "parts": {}, "taken": 0})
            if slot["op"] != op:
                self.fail(LoopError(f"collective {seq}: rank {me} calls {op}, another rank "
                                    f"{slot['op']}"))
                self._cond.notify_all()
                raise self.error
            slot["parts"][me] = part
            self._cond.notify_all()

        def finish():
            with self._cond:
                self._wait_for(lambda: len(slot["parts"]) == self.world,
                               f"collective {seq} ({op})")
                parts = [slot["parts"][r] for r in range(self.world)]
                slot["taken"] += 1
                if slot["taken"] == self.world:
                    del self._coll[seq]
            apply(parts)
        req = _Pending(finish)
        if async_op:
            return req
        req.wait()
        return None

    @staticmethod
    def _sum(parts):
        """THE summation order: ascending rank, in the tensors' precision."""
        acc = parts[0]
        for p in parts[1:]:
            acc = acc + p
        return acc

    @staticmethod
    def _check_op(op):
        if op != ReduceOp.SUM:
            raise LoopError(f"only ReduceOp.SUM is implemented, not {op!r}")

    @staticmethod
    def _flat(t, what):
        if not t.is_contiguous():
            raise LoopError(f"{what} must be contiguous")
        return t.view(-1)

    def barrier(self, group=None, async_op=False):
        return self._collective("barrier", None, lambda parts: None, async_op)

    def all_gather_into_tensor(self, output_tensor, input_tensor, group=None, async_op=False):
        W, n = self.world, input_tensor.numel()
        out = self._flat(output_tensor, "all_gather_into_tensor's output")
        if out.numel() != W * n or output_tensor.dtype != input_tensor.dtype:
            raise LoopError(f"all_gather_into_tensor: output of {out.numel()} for {W} x {n}")

        def apply(parts):
            for r, p in enumerate(parts):
                out[r * n:(r + 1) * n].copy_(p.reshape(-1))
        return self._collective("all_gather_into_tensor", self._payload(input_tensor), apply,
                                async_op)

    def broadcast(self, tensor, src, group=None, async_op=False):
        me = self.get_rank()

        def apply(parts):
            if me != src:
                p = parts[src]
                if p is None or p.numel() != tensor.numel() or p.dtype != tensor.dtype:
                    raise LoopError(f"broadcast from rank {src}: sizes differ between ranks")
                tensor.copy_(p.view(tensor.shape))
        return self._collective(f"broadcast/{src}", self._payload(tensor) if me == src else None,
                                apply, async_op)

    def _same(self, parts, t, what):
        for p in parts:
            if p.numel() != t.numel() or p.dtype != t.dtype:
                raise LoopError(f"{what}: sizes differ between ranks")

    def all_reduce(self, tensor, op=ReduceOp.SUM, group=None, async_op=False):
        self._check_op(op)

        def apply(parts):
            self._same(parts, tensor, "all_reduce")
            tensor.copy_(self._sum(parts).view(tensor.shape))
        return self._collective("all_reduce", self._payload(tensor), apply, async_op)

    def reduce(self, tensor, dst, op=ReduceOp.SUM, group=None, async_op=False):
        self._check_op(op)
        me = self.get_rank()

        def apply(parts):
            self._same(parts, tensor, "reduce")
            if me == dst:
                tensor.copy_(self._sum(parts).view(tensor.shape))
        return self._collective(f"reduce/{dst}", self._payload(tensor), apply, async_op)

    def reduce_scatter_tensor(self, output, input, op=ReduceOp.SUM, group=None, async_op=False):
        self._check_op(op)
        me, W, q = self.get_rank(), self.world, output.numel()
        if input.numel() != W * q or input.dtype != output.dtype:
            raise LoopError(f"reduce_scatter_tensor: input of {input.numel()} for {W} x {q}")
        self._flat(input, "reduce_scatter_tensor's input")

        def apply(parts):
            self._same(parts, input, "reduce_scatter_tensor")
            output.copy_(self._sum([p.view(-1)[me * q:(me + 1) * q] for p in parts])
                         .view(output.shape))
        return self._collective("reduce_scatter_tensor", self._payload(input), apply, async_op)

    def gather(self, tensor, gather_list=None, dst=0, group=None, async_op=False):
        me = self.get_rank()
        if (me == dst) != (gather_list is not None):
            raise LoopError("gather: gather_list on the destination rank and only there")
        if me == dst and len(gather_list) != self.world:
            raise LoopError("gather: one destination tensor per rank")

        def apply(parts):
            if me == dst:
                for t, p in zip(gather_list, parts):
                    if p.numel() != t.numel() or p.dtype != t.dtype:
                        raise LoopError("gather: sizes differ between ranks")
                    t.copy_(p.view(t.shape))
        return self._collective(f"gather/{dst}", self._payload(tensor), apply, async_op)


def run_ranks(world, fn, loop=None, device=None, limit=120.0):
    """Run ``fn(rank)`` in ``world`` daemon threads over ``loop`` (default:
    the LoopDist standing in for ``feddct_amd.dist.dist``) and return the W
    results.  The first exception of any rank is re-raised here; ranks still
    running after ``limit`` seconds make a TimeoutError.  No retries."""
    if loop is None:
        import feddct_amd.dist as D
        loop = D.dist
    if not isinstance(loop, LoopDist) or loop.world != world:
        raise LoopError(f"run_ranks({world}) needs a LoopDist of that world in place of "
                        f"feddct_amd.dist.dist")
    results = [None] * world

    def body(rank):
        loop._bind(rank)
        with loop._cond:
            try:
                if device is not None and torch.device(device).type == "cuda":
                    torch.cuda.set_device(device)
                results[rank] = fn(rank)
            except BaseException as e:  # noqa: BLE001 - handed to the driver
                loop.fail(e)
                loop._cond.notify_all()

    threads = [threading.Thread(target=body, args=(r,), daemon=True, name=f"loop-rank{r}")
               for r in range(world)]
    for t in threads:
        t.start()
    end = time.monotonic() + limit
    for t in threads:
        t.join(max(0.0, end - time.monotonic()))
    alive = [t.name for t in threads if t.is_alive()]
    if alive and loop.error is None:
        loop.fail(TimeoutError(f"{alive} still running after {limit} s"))
    if loop.error is not None:
        raise loop.error
    return results
