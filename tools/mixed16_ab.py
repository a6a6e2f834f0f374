"""The mixed round (fp32 master global over 16-bit clients)
beside the pure 16-bit round, one process, same buffers: wrn16_8 C10's shapes
in bf16 (or fp16), clients carved from one slab as the product places them.
A sibling of tools/h16_ab.py, whose warm-up, rotation and timing it keeps.

    python tools/mixed16_ab.py kernel [--n 5,20,24] [--dtype bfloat16] [--rounds 7]
        per N, launches interleaved variant by variant over several rounds
        (HIP events around a run of back-to-back calls): the pure 16-bit
        reduce and its flat broadcast (fa_plan_create_elem), the mixed reduce
        (wide store) and the narrowing broadcast (fa_plan_create_elem_out);
        us and GB/s of each launch's own algorithmic bytes
            16-bit reduce     N*2*E + 2*E + int64      flat broadcast    2*E + N*2*E + int64
            mixed reduce      N*2*E + 4*E + int64      mixed broadcast   4*E + N*2*E + int64
        (int64: (N+1) * 8 bytes per element), the measured ratio of the mixed
        round (reduce + broadcast) to the 16-bit one beside the byte ratio
        (4N+8)/(4N+4), and each launch's own ratio.
    python tools/mixed16_ab.py dropin [--tree DIR --label NAME] [--n 20] [--dtype bfloat16]
        wall time of one server_aggregate round of an fp32 global + N
        model.bfloat16() clients on the GPU, through the public call only, so
        the same script measures another checkout of the package (--tree):
        median of --calls calls after 3.

Each record is one JSON line, appended to --out (default
profiles/mixed16_<leg>.jsonl) and printed.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


# ------------------------------------------------------------ kernel leg ----
def kernel_leg(args):
    from feddct_amd import _lib, slab, synth
    from feddct_amd.layout import KIND_I64, BucketLayout
    from feddct_amd.workload import load_manifest
    tdt = getattr(torch, args.dtype)
    man = load_manifest(args.layout)
    lay32 = BucketLayout.from_manifest(man)
    lay16 = BucketLayout([(e["key"], e["shape"], e["dtype"] if e["dtype"] == "int64"
                           else args.dtype) for e in man["keys"]], native16=True)
    master = BucketLayout([(e["key"], e["shape"], e["dtype"]) for e in man["keys"]],
                          master16=True)
    assert lay16.native16 and master.f32_numel == lay16.f32_numel
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = _lib.lib

    def client(c):
        f32 = torch.zeros(lay32.f32_numel, dtype=torch.float32, device=dev)
        h16 = slab.carve(lay16.f32_numel, tdt, dev)
        i64 = torch.zeros(max(lay32.i64_numel, 1), dtype=torch.int64, device=dev)
        for j, e in enumerate(man["keys"]):
            s, t = lay32.by_key[e["key"]], lay16.by_key[e["key"]]
            if s.kind == KIND_I64:
                _lib.check(L.fa_synth_fill_i64(i64[s.offset:].data_ptr(), s.numel, j, c, 0, st))
            else:
                mu, sg = synth.key_params(e["key"], tuple(e["shape"]), e["dtype"])
                _lib.check(L.fa_synth_fill_f32(f32[s.offset:].data_ptr(), s.numel, j, c, mu, sg,
                                               0, st))
                h16[t.offset:t.offset + t.numel] = f32[s.offset:s.offset + s.numel].to(tdt)
        return h16, i64

    elem = _lib.ELEM_OF_DTYPE[tdt]
    pure = _lib.Plan(lay16.segs32, lay16.f32_numel, lay16.segs64, lay16.i64_numel, elem=elem)
    mixed = _lib.Plan(lay16.segs32, lay16.f32_numel, lay16.segs64, lay16.i64_numel, elem=elem,
                      out_elem=_lib.FA_ELEM_F32)
    variants = {"h16_reduce": (pure, "o16", 0), "h16_bcast": (pure, "o16", _lib.FA_F_BCAST_ONLY),
                "mixed_reduce": (mixed, "o32", 0),
                "mixed_bcast": (mixed, "o32", _lib.FA_F_BCAST_ONLY)}
    E, I = lay16.f32_data_elems, lay16.i64_data_elems
    for n in args.n:
        # enough rotating client sets that a set's bytes exceed the 256 MB
        # last-level cache several times over before it comes round again
        rot = max(1, -(-(1 << 30) // (n * 2 * lay16.f32_numel)))
        sets = []
        for _ in range(rot):
            slab.release()
            with slab.expecting(n + 3):
                cl = [client(c) for c in range(n)]
                o16 = slab.carve(lay16.f32_numel, tdt, dev)
                o32 = slab.carve(master.f32_numel, torch.float32, dev)
            o64 = torch.zeros_like(cl[0][1])
            sets.append({"p16": _lib.ptr_array([c[0].data_ptr() for c in cl]),
                         "p64": _lib.ptr_array([c[1].data_ptr() for c in cl]),
                         "o16": o16, "o32": o32, "o64": o64, "keep": cl})
        nbytes = {"h16_reduce": n * 2 * E + 2 * E, "h16_bcast": 2 * E + n * 2 * E,
                  "mixed_reduce": n * 2 * E + 4 * E, "mixed_bcast": 4 * E + n * 2 * E}
        nbytes = {k: v + (n + 1) * 8 * I for k, v in nbytes.items()}

        def call(name, i):
            s = sets[i % rot]
            plan, o, flags = variants[name]
            _lib.check(L.fa_reduce(plan.handle, s["p16"], s["p64"], n, None, s[o].data_ptr(),
                                   s["o64"].data_ptr(), flags, st), "fa_reduce")
        reps = (60 if n > 10 else 200) * rot
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for name in variants:
                for i in range(3 * rot):
                    call(name, i)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(reps):
                    call(name, i)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / reps * 1e3)
        # after the last round every client holds its set's broadcast global:
        # the two broadcasts gave the clients the same bits
        same = all(torch.equal(s["keep"][0][0].view(torch.int16), s["o32"].to(tdt).view(torch.int16))
                   for s in sets)
        rec = {"exp": "mixed16_ab_kernel", "layout": args.layout, "dtype": args.dtype, "n": n,
               "rot": rot, "reps": reps, "rounds": args.rounds, "elems": E,
               "clients_hold_narrowed_global": bool(same)}
        med = {k: median(v) for k, v in times.items()}
        for name in variants:
            rec[name] = {"us_median": round(med[name], 2), "us_min": round(min(times[name]), 2),
                         "us_max": round(max(times[name]), 2), "alg_bytes": nbytes[name],
                         "gbps": round(nbytes[name] / med[name] / 1e3, 1)}
        rec["ratio_round_measured"] = round((med["mixed_reduce"] + med["mixed_bcast"])
                                            / (med["h16_reduce"] + med["h16_bcast"]), 4)
        rec["ratio_round_bytes"] = round((4 * n + 8) / (4 * n + 4), 4)
        rec["ratio_reduce_measured"] = round(med["mixed_reduce"] / med["h16_reduce"], 4)
        rec["ratio_reduce_bytes"] = round(nbytes["mixed_reduce"] / nbytes["h16_reduce"], 4)
        rec["ratio_bcast_measured"] = round(med["mixed_bcast"] / med["h16_bcast"], 4)
        rec["ratio_bcast_bytes"] = round(nbytes["mixed_bcast"] / nbytes["h16_bcast"], 4)
        # the widest relative spread (max - min) / median among the four launches
        rec["spread"] = round(max((max(v) - min(v)) / med[k] for k, v in times.items()), 4)
        emit(rec, args.out or os.path.join(ROOT, "profiles", "mixed16_kernel.jsonl"))
        del sets
        torch.cuda.empty_cache()


# ----------------------------------------------------------- drop-in leg ----
class ManifestModule(torch.nn.Module):
    """A module whose state_dict has a manifest's keys, shapes and dtypes."""

    def __init__(self, manifest):
        super().__init__()
        for i, e in enumerate(manifest["keys"]):
            t = torch.zeros(e["shape"], dtype=getattr(torch, e["dtype"]))
            name = f"k{i}_" + e["key"].replace(".", "_")
            if t.is_floating_point():
                self.register_parameter(name, torch.nn.Parameter(t))
            else:
                self.register_buffer(name, t)


def dropin_leg(args):
    import feddct_amd
    from feddct_amd.workload import load_manifest
    tdt = getattr(torch, args.dtype)
    man = load_manifest(args.layout)
    n = args.n[0]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gen = torch.Generator().manual_seed(1)

    def model(c, dt):
        m = ManifestModule(man)
        with torch.no_grad():
            for v in m.state_dict().values():
                if v.is_floating_point():
                    v.copy_(torch.randn(v.shape, generator=gen) * 0.05)
                else:
                    v.fill_(100 + c)
        return m.to(dt).to(dev)
    g = model(0, torch.float32)           # the fp32 master global
    clients = [model(c + 1, tdt) for c in range(n)]
    for _ in range(3):     # the first call binds the modules
        feddct_amd.server_aggregate(g, clients)
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        feddct_amd.server_aggregate(g, clients)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    a, c = getattr(g, "_fa_arena", None), getattr(clients[0], "_fa_arena", None)
    rb = feddct_amd.aggregate.engine()._round
    rec = {"exp": "mixed16_ab_dropin", "tree": args.label,
           "layout": args.layout, "dtype": args.dtype, "n": n, "calls": args.calls,
           "global_bucket_dtype": str(a.f32.dtype) if a is not None else None,
           "client_bucket_dtype": str(c.f32.dtype) if c is not None else None,
           "client_staged_keys": len(c._packed) if c is not None else None,
           "bound_native_round": bool(rb is not None and rb.native is not None),
           "wall_us_median": round(median(ts), 1), "wall_us_min": round(min(ts), 1),
           "wall_us_max": round(max(ts), 1)}
    emit(rec, args.out or os.path.join(ROOT, "profiles", "mixed16_dropin.jsonl"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["kernel", "dropin"])
    ap.add_argument("--n", default=None)
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float16"])
    ap.add_argument("--layout", default="wrn16_8_c10")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--tree", default=ROOT, help="checkout whose feddct_amd package is measured")
    ap.add_argument("--label", default="this tree", help="name of --tree in the record")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.n = [int(x) for x in (args.n or ("5,20,24" if args.leg == "kernel" else "20")).split(",")]
    sys.path.insert(0, os.path.abspath(args.tree))
    if not torch.cuda.is_available():
        raise SystemExit("mixed16_ab: no HIP device (a measurement needs the GPU)")
    (kernel_leg if args.leg == "kernel" else dropin_leg)(args)


if __name__ == "__main__":
    main()
