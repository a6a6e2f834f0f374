"""What feddct_amd.comm's native wrappers hand to the C ABI, recorded without
the library: ``Recorder`` stands in for ``comm.lib()`` (every ``fa_*``
attribute logs its normalised arguments and returns 0), ``cases()`` lists the
argument sets and ``record(C, install)`` runs them against a comm module.
tests/test_comm_wrappers_cpu.py holds the module to the calls recorded from
the commit before the wrappers were folded into one base
(tests/golden/comm_wrapper_calls.json, written by
tests/golden/make_comm_wrapper_golden.py, which shares this module).

Nothing here touches a GPU: tensors are CPU tensors, the communicator is a
``Comm`` made without fa_comm_init_rank, ``step`` gets an explicit stream.

Normalisation: ints stay ints; a handle (c_void_p) is its value; a ctypes
array is the list of its values (fa_seg arrays: [offset, numel] pairs); a
``byref(FaShardIO)`` is a dict of its fields with every tensor address
replaced by the tensor's name in the case (``local32[1]``, ``out64``, ...);
any other ``byref`` is an out-parameter, logged as ``out:<ctype>``."""
import ctypes
import gc
import inspect
import itertools

import torch

COMM_HANDLE = 0xC0
STREAM = 0x5EED
N_TOTAL = 5

PLANS = ["ShardPlan", "StripePlan", "ChainPlan", "BlockPlan", "MultiPlan"]
AGGREGATORS = ["NativeShardedAggregator", "NativeStripedAggregator", "NativeChainedAggregator",
               "NativeBlockedAggregator", "NativeAggregator"]
TAKES_COUNTS = AGGREGATORS[1:]
TAKES_NCHUNKS = [a for a in AGGREGATORS if a != "NativeBlockedAggregator"]
CREATE = {"ShardPlan": "fa_shard_plan_create_ex", "StripePlan": "fa_stripe_plan_create_ex",
          "ChainPlan": "fa_chain_plan_create", "BlockPlan": "fa_block_plan_create",
          "MultiPlan": "fa_multi_plan_create"}
DESTROY = {"ShardPlan": "fa_shard_plan_destroy", "StripePlan": "fa_stripe_plan_destroy",
           "ChainPlan": "fa_chain_plan_destroy", "BlockPlan": "fa_block_plan_destroy",
           "MultiPlan": "fa_multi_plan_destroy"}
REDUCE = dict(zip(AGGREGATORS, ["fa_reduce_sharded", "fa_reduce_striped", "fa_reduce_chained",
                                "fa_reduce_blocked", "fa_reduce_multi"]))

_F32 = [{"key": "a", "shape": [5], "dtype": "float32"},
        {"key": "b", "shape": [70], "dtype": "float32"},
        {"key": "c", "shape": [3], "dtype": "float32"}]
MANIFESTS = {"i64": {"keys": _F32[:2] + [{"key": "n", "shape": [], "dtype": "int64"}] + _F32[2:]
                     + [{"key": "m", "shape": [], "dtype": "int64"}]},
             "noi64": {"keys": _F32}}
WORLDS = [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]
WEIGHTS = ["none", "given", "empty"]
# explicit shard counts per world size, each with a rank that holds no slot
COUNTS = {1: [[5]], 2: [[5, 0], [1, 4]], 3: [[2, 0, 3], [3, 2, 0]]}


class Recorder:
    """The stand-in for libfedagg_comm.so.  ``world``, ``rank``: what
    fa_comm_info reports; ``mode``, ``chunks``: what fa_multi_plan_mode and
    fa_multi_plan_chunks report; ``fail``: entry point -> its return code.
    ``names``: tensor address -> name; ``behind``: the element counts behind
    FaShardIO's c32, c64 and weights pointers (the library knows them from
    the plan)."""

    def __init__(self, world=1, rank=0, mode=2, chunks=5, fail=None):
        self.log = []
        self.world, self.rank, self.mode, self.chunks = world, rank, mode, chunks
        self.fail = dict(fail or {})
        self.names, self.behind = {}, {}
        self._handles = itertools.count(1)

    def __getattr__(self, name):
        if not name.startswith("fa_"):
            raise AttributeError(name)

        def call(*args):
            self.log.append([name, [self._norm(a) for a in args]])
            rc = self.fail.get(name, 0)
            if rc == 0:
                self._fill(name, [a._obj for a in args if _is_byref(a)])
            return rc
        return call

    def _fill(self, name, outs):
        if "_plan_create" in name:
            outs[-1].value = 0x1000 * next(self._handles)
        elif name == "fa_comm_info":
            for o, v in zip(outs, (self.world, self.rank, 0)):
                o.value = v
        elif name == "fa_multi_plan_mode":
            outs[0].value = self.mode
        elif name == "fa_multi_plan_chunks":
            outs[0].value = self.chunks

    def _norm(self, a):
        if a is None or type(a) in (int, float):
            return a
        if isinstance(a, ctypes.c_void_p):
            return a.value
        if isinstance(a, ctypes.Array):
            if issubclass(a._type_, ctypes.Structure):
                return [[getattr(x, f) for f, _ in x._fields_] for x in a]
            return list(a)
        if _is_byref(a):
            o = a._obj
            return self._io(o) if type(o).__name__ == "FaShardIO" else "out:" + type(o).__name__
        raise TypeError(f"no rule to record {a!r}")

    def _io(self, io):
        def ptrs(addr, n):
            if addr is None:
                return None
            return [self.names[p] for p in (ctypes.c_void_p * n).from_address(addr)]
        w = io.weights
        return {"c32": ptrs(io.c32, self.behind["c32"]), "c64": ptrs(io.c64, self.behind["c64"]),
                "weights": (None if w is None else
                            list((ctypes.c_float * self.behind["weights"]).from_address(w))),
                "out32": self.names[io.out32],
                "out64": None if io.out64 is None else self.names[io.out64],
                "stream": io.stream}


def _is_byref(a):
    return type(a).__name__ == "CArgObject"


def _default_counts(n_total, world):
    return [n_total // world + (1 if r < n_total % world else 0) for r in range(world)]


def _name(kind, **parts):
    return kind + "/" + "/".join(f"{k}={parts[k]}" for k in parts)


def _agg(cls, world, rank, layout="i64", final="reduce", weights="none", n_total=N_TOTAL,
         nlocal=None, rec=None, **kw):
    """An aggregator case: ``kw`` goes to the constructor beside ``final``;
    ``nlocal``: the clients held, where not the shard's count; ``rec``:
    Recorder arguments."""
    d = dict(kind="agg", cls=cls, world=world, rank=rank, layout=layout, final=final,
             weights=weights, n_total=n_total, nlocal=nlocal, rec=rec or {}, kw=kw)
    d["name"] = _name(cls, w=world, r=rank, lay=layout, final=final, wt=weights, n=n_total,
                      nlocal=nlocal, rec=d["rec"], kw=kw)
    return d


def cases():
    out = []
    # every aggregator at every rank of worlds 1-3, both layouts, both finals;
    # the weights kinds cycle (every class meets each kind on each layout)
    grid = itertools.product(AGGREGATORS, WORLDS, MANIFESTS, ("reduce", "allreduce"))
    for i, (cls, (w, r), lay, final) in enumerate(grid):
        out.append(_agg(cls, w, r, lay, final, WEIGHTS[i % 3]))
    for cls in TAKES_COUNTS:            # explicit counts, a rank without slots among them
        for w, r in WORLDS:
            for counts in COUNTS[w]:
                for final in ("reduce", "allreduce"):
                    out.append(_agg(cls, w, r, final=final, weights="given", counts=counts))
    for cls in AGGREGATORS:             # fewer slots than ranks: the default counts end in 0
        out += [_agg(cls, 3, r, n_total=2) for r in range(3)]
    for cls in TAKES_NCHUNKS:
        out += [_agg(cls, w, r, nchunks=k) for w, r in ((1, 0), (2, 1)) for k in (0, 3)]
    for w, r in WORLDS:
        for final in ("reduce", "allreduce"):
            out.append(_agg(AGGREGATORS[0], w, r, final=final, exchange=1))  # FA_XCHG_RS_GATHER
            out.append(_agg("NativeAggregator", w, r, final=final, exact=False, rec={"mode": 0}))
    for cls in AGGREGATORS:             # an explicit root
        out += [_agg(cls, 3, 1, final=f, root=root) for f in ("reduce", "allreduce")
                for root in (0, 2)]
    for mode, k in ((0, 1), (1, 4), (2, 16), (3, 1)):   # what the multi plan reads back
        out.append(_agg("NativeAggregator", 2, 0, rec={"mode": mode, "chunks": k}))
    # ---- argument sets that raise
    for cls in AGGREGATORS:
        out.append(_agg(cls, 2, 0, final="sum"))
        out.append(_agg(cls, 2, 0, nlocal=4))
        out.append(_agg(cls, 3, 2, nlocal=0))
    for cls in TAKES_COUNTS:
        out.append(_agg(cls, 2, 0, nlocal=3, counts=[3, 3]))        # sum(counts) != n_total
        out.append(_agg(cls, 2, 1, nlocal=1, counts=[5]))           # shorter than the world
        out.append(_agg(cls, 2, 0, nlocal=5, counts=[5]))
        out.append(_agg(cls, 2, 0, nlocal=3, counts=[3, 2, 0]))     # longer than the world
    # ---- a failing entry point: the label in FedaggError's text
    for cls, plan in zip(AGGREGATORS, PLANS):
        out.append(_agg(cls, 2, 1, rec={"fail": {CREATE[plan]: -3}}))
        out.append(_agg(cls, 2, 1, rec={"fail": {REDUCE[cls]: -6}}))
    out += [_agg("NativeAggregator", 2, 1, rec={"fail": {f: -1}})
            for f in ("fa_multi_plan_mode", "fa_multi_plan_chunks")]
    # ---- the plan classes on their own: defaults, explicit arguments, collection
    extra = {"ShardPlan": [{}, {"nchunks": 3, "exchange": 1}], "StripePlan": [{}, {"nchunks": 3}],
             "ChainPlan": [{}, {"nchunks": 3}], "BlockPlan": [{}],
             "MultiPlan": [{}, {"nchunks": 3, "exact": False, "root_all": True},
                           {"root_all": True}]}
    for plan in PLANS:
        for lay in MANIFESTS:
            for kw in extra[plan]:
                out.append(dict(kind="plan", cls=plan, layout=lay, kw=kw,
                                name=_name(plan, lay=lay, kw=kw)))
    # ---- the host-only helpers that marshal a layout and counts
    for lay in MANIFESTS:
        for fn, kw in (("multi_select", {"detail": True}),
                       ("multi_select", {"exact": False, "root_all": True}),
                       ("round_model", {"mode": 2}),
                       ("round_model", {"mode": 0, "nchunks": 3, "exchange": 1, "root": -1,
                                        "weighted": True}),
                       ("describe", {"mode": 1, "rank": 1}),
                       ("describe", {"mode": 3, "rank": 0, "nchunks": 2, "root": 2,
                                     "weighted": True})):
            out.append(dict(kind="host", fn=fn, layout=lay, kw=kw,
                            name=_name(fn, lay=lay, kw=kw)))
    out.append(dict(kind="host", fn="multi_select", layout=None, kw={"root_all": True},
                    name=_name("multi_select", lay=None, kw={"root_all": True})))
    assert len({c["name"] for c in out}) == len(out)
    return out


def _error(C, e):
    """An exception as recorded: FedaggError without the library's own
    message (what fa_last_error holds depends on the process's earlier calls)."""
    s = str(e)
    if isinstance(e, C._lib.FedaggError):
        s = s.split("): ")[0] + ")"
    return f"{type(e).__name__}: {s}"


def _run_agg(C, c, install, layout):
    world, rank, n_total, kw = c["world"], c["rank"], c["n_total"], dict(c["kw"])
    counts = kw.get("counts") or _default_counts(n_total, world)
    n = c["nlocal"] if c["nlocal"] is not None else counts[rank]
    local32 = [torch.zeros(max(64, layout.f32_numel)) for _ in range(n)]
    local64 = [torch.zeros(max(1, layout.i64_numel), dtype=torch.int64) for _ in range(n)]
    out32 = torch.zeros(max(64, layout.f32_numel))
    out64 = torch.zeros(max(1, layout.i64_numel), dtype=torch.int64)
    weights = {"none": None, "given": [(j + 1) / 8 for j in range(n)], "empty": []}[c["weights"]]
    rec = Recorder(world, rank, **c["rec"])
    rec.behind = {"c32": n, "c64": n, "weights": len(weights or ())}
    for j in range(n):
        rec.names[local32[j].data_ptr()] = f"local32[{j}]"
        rec.names[local64[j].data_ptr()] = f"local64[{j}]"
    rec.names[out32.data_ptr()], rec.names[out64.data_ptr()] = "out32", "out64"
    assert len(rec.names) == 2 * n + 2
    install(rec)
    comm = object.__new__(C.Comm)
    comm.handle, comm.nranks, comm.rank = ctypes.c_void_p(COMM_HANDLE), world, rank
    res = {"error": None}
    try:
        agg = getattr(C, c["cls"])(layout, local32, local64, n_total, out32, out64, comm,
                                   final=c["final"], weights=weights, **kw)
        keep = agg._keep
        res["attrs"] = {"root": agg.root, "handle": agg.plan.handle.value,
                        "mode": getattr(agg, "mode", None),
                        "nchunks": getattr(agg, "nchunks", None),
                        "plan_comm": agg.plan.comm is comm,
                        "keep": (len(keep) == 4 and keep[0] is local32 and keep[1] is local64
                                 and keep[2] is out32 and keep[3] is out64)}
        agg.step(stream=STREAM)
        agg.step(stream=STREAM + 1)
    except (ValueError, IndexError, C._lib.FedaggError) as e:
        res["error"] = _error(C, e)
    # the plan holds its communicator: dropping the caller's reference first
    # must still see the plan destroyed before the communicator
    agg = keep = None
    del comm
    res["calls"] = rec.log
    return res


def _run_plan(C, c, install, layout):
    cls = getattr(C, c["cls"])
    rec = Recorder(2, 1)
    install(rec)
    comm = object.__new__(C.Comm)
    comm.handle, comm.nranks, comm.rank = ctypes.c_void_p(COMM_HANDLE), 2, 1
    res, marks = {}, [0]

    def since():
        marks.append(len(rec.log))
        return rec.log[marks[-2]:]
    p = cls(comm, layout, [3, 2], **c["kw"])
    res["attrs"] = {"handle": p.handle.value, "plan_comm": p.comm is comm,
                    "mode": getattr(p, "mode", None), "nchunks": getattr(p, "nchunks", None)}
    res["profile"] = C.plan_profile(p)
    res["create"] = since()
    del p                               # (no cycle holds a plan: the last reference frees it)
    res["collected"] = since()          # one call of the plan's own destroy, its handle
    gc.collect()
    res["collected_again"] = since()    # nothing
    q = cls(comm, layout, [3, 2], **c["kw"])
    since()
    q.__del__()
    q.__del__()
    del q
    res["finalised_twice"] = since()    # one call again
    rec.fail[CREATE[c["cls"]]] = -2     # a refused create leaves nothing to destroy
    try:
        cls(comm, layout, [3, 2], **c["kw"])
    except C._lib.FedaggError as e:
        res["refused"] = _error(C, e)
    res["refused_calls"] = [f for f, _ in since()]
    del comm
    res["comm"] = since()
    return res


def _run_host(C, c, install, layout):
    rec = Recorder()
    install(rec)
    kw = dict(c["kw"], layout=layout)
    counts = [2, 0, 3]
    if c["fn"] == "multi_select":
        got = C.multi_select(counts, **kw)
    else:
        got = getattr(C, c["fn"])(kw.pop("mode"), kw.pop("layout"), counts, **kw)
    return {"returns": got, "calls": rec.log}


def signatures(C):
    return {n: str(inspect.signature(getattr(C, n).__init__)) for n in PLANS + AGGREGATORS}


def record(C, install):
    """name -> what the case logged, for every case, on comm module ``C``;
    ``install(recorder)`` puts the recorder in ``C._clib``'s place."""
    layouts = {k: C.BucketLayout.from_manifest(m) for k, m in MANIFESTS.items()}
    layouts[None] = None
    run = {"agg": _run_agg, "plan": _run_plan, "host": _run_host}
    return {c["name"]: run[c["kind"]](C, c, install, layouts[c["layout"]]) for c in cases()}
