"""The torch-GPU-order reduce over 16-bit buckets against its two neighbours,
one process, same buffers: wrn16_8 C10's shapes cast to bf16
(or fp16), clients carved from one slab as the product places them.

    python tools/tgpu16_ab.py kernel [--n 5,20,32,64] [--dtype bfloat16] [--rounds 7]
        per N, launches interleaved variant by variant over several rounds
        (HIP events around a run of back-to-back calls after a warm-up;
        client sets rotated so at least 1 GiB is read before a set repeats):
        the fp32 torch-GPU-order reduce of the same element count
        (fa_plan_create_order), the CPU-order 16-bit reduce
        (fa_plan_create_elem) and the torch-GPU-order 16-bit reduce
        (fa_plan_create_order_elem); us, GB/s of each variant's own
        algorithmic bytes ((N + 1) * element size per element + the int64
        keys), and the ratio to the fp32 time.
    python tools/tgpu16_ab.py dropin [--tree DIR --label NAME] [--native16 1] [--n 20]
        wall time of one server_aggregate round under the torch-GPU order on
        N model.bfloat16() clients + global on the GPU, through the public
        call only, so the same script measures another checkout of the
        package (--tree; --native16 0 there: the staged round).

    --master 1 on either leg: an fp32 master global over the 16-bit clients
        (DESIGN §4.13).  kernel: the 16-bit torch-GPU-order reduce, the
        CPU-order mixed reduce (fa_plan_create_elem_out) and the
        torch-GPU-order mixed reduce (fa_plan_create_order_elem_out) of the
        same client buckets, the mixed ones into an fp32 bucket (4 B per
        element written where the 16-bit one writes 2), and the ratio to the
        16-bit torch-GPU-order time.  dropin: the global stays fp32;
        --native16 2 sets native16_master=True too (--native16 1 on a
        checkout from before that option: the staged round).

Each record is one JSON line, appended to --out (default
profiles/tgpu16_<leg>.jsonl, with --master profiles/tgpu16_master_<leg>.jsonl)
and printed.
"""
import argparse
import ctypes
import hashlib
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
    assert lay16.native16
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = _lib.lib
    elem = _lib.ELEM_OF_DTYPE[tdt]

    def client(c):
        f32 = slab.carve(lay32.f32_numel, torch.float32, dev)
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
        return f32, h16, i64

    for n in args.n:
        if args.master:
            plans = {
                "h16_tgpu": _lib.Plan.for_order(lay16.segs32, lay16.f32_numel, lay16.segs64,
                                                lay16.i64_numel, n=n, elem=elem),
                "mix_cpu": _lib.Plan(lay16.segs32, lay16.f32_numel, lay16.segs64,
                                     lay16.i64_numel, elem=elem, out_elem=_lib.FA_ELEM_F32),
                "mix_tgpu": _lib.Plan.for_order(lay16.segs32, lay16.f32_numel, lay16.segs64,
                                                lay16.i64_numel, n=n, elem=elem,
                                                out_elem=_lib.FA_ELEM_F32),
            }
        else:
            plans = {
                "f32_tgpu": _lib.Plan(lay32.segs32, lay32.f32_numel, lay32.segs64,
                                      lay32.i64_numel, order=_lib.FA_ORDER_TORCH_GPU, n=n),
                "h16_cpu": _lib.Plan(lay16.segs32, lay16.f32_numel, lay16.segs64,
                                     lay16.i64_numel, elem=elem),
                "h16_tgpu": _lib.Plan.for_order(lay16.segs32, lay16.f32_numel, lay16.segs64,
                                                lay16.i64_numel, n=n, elem=elem),
            }
        rot = max(1, -(-(1 << 30) // (n * 2 * lay16.f32_numel)))
        sets = []
        for _ in range(rot):
            slab.release()
            with slab.expecting(2 * n + 3):
                cl = [client(c) for c in range(n)]
                o32 = slab.carve(lay32.f32_numel, torch.float32, dev)
                o16 = slab.carve(lay16.f32_numel, tdt, dev)
                # the master global's bucket: fp32 at the 16-bit layout's offsets
                om = slab.carve(lay16.f32_numel, torch.float32, dev)
            o64 = torch.zeros_like(cl[0][2])
            sets.append({
                "f32": (_lib.ptr_array([c[0].data_ptr() for c in cl]), o32),
                "h16": (_lib.ptr_array([c[1].data_ptr() for c in cl]), o16),
                "mix": (_lib.ptr_array([c[1].data_ptr() for c in cl]), om),
                "i64": (_lib.ptr_array([c[2].data_ptr() for c in cl]), o64), "keep": cl})

        def call(name, i):
            s = sets[i % rot]
            p, o = s[name[:3]]
            p64, o64 = s["i64"]
            _lib.check(L.fa_reduce(plans[name].handle, p, p64, n, None, o.data_ptr(),
                                   o64.data_ptr(), 0, st), "fa_reduce")
        reps = (60 if n > 10 else 200) * rot
        times = {k: [] for k in plans}
        for _ in range(args.rounds):
            for name in plans:
                for i in range(3 * rot):
                    call(name, i)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(reps):
                    call(name, i)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / reps * 1e3)
        rec = {"exp": "tgpu16_ab_kernel", "tree": args.label, "layout": args.layout, "dtype": args.dtype, "n": n,
               "rot": rot, "reps": reps, "rounds": args.rounds, "elems": lay16.f32_data_elems,
               "tiles": {k: p.info["ntiles"] for k, p in plans.items()}}
        base = "h16_tgpu" if args.master else "f32_tgpu"
        base_med = median(times[base])
        for name in plans:
            nb = (lay32 if name.startswith("f32") else lay16).algorithmic_bytes(n)
            if name.startswith("mix"):   # the result is written in fp32
                nb += 2 * lay16.f32_data_elems
            med = median(times[name])
            rec[name] = {"us_median": round(med, 2), "us_min": round(min(times[name]), 2),
                         "us_max": round(max(times[name]), 2), "alg_bytes": nb,
                         "gbps": round(nb / med / 1e3, 1),
                         "vs_h16_tgpu" if args.master else "vs_f32": round(med / base_med, 4)}
        emit(rec, args.out or os.path.join(
            ROOT, "profiles", "tgpu16_master_kernel.jsonl" if args.master else "tgpu16_kernel.jsonl"))
        del sets, plans
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

    def model(c, fp32=False):
        m = ManifestModule(man)
        with torch.no_grad():
            for v in m.state_dict().values():
                if v.is_floating_point():
                    v.copy_(torch.randn(v.shape, generator=gen) * 0.05)
                else:
                    v.fill_(100 + c)
        return (m if fp32 else m.to(tdt)).to(dev)
    g = model(0, fp32=bool(args.master))
    clients = [model(c + 1) for c in range(n)]
    if args.native16 == 2:
        feddct_amd.set_summation_order("torch_gpu", native16=True, native16_master=True)
    elif args.native16:
        feddct_amd.set_summation_order("torch_gpu", native16=True)
    else:   # (a checkout from before the option: the staged round)
        feddct_amd.set_summation_order("torch_gpu")
    for _ in range(3):     # the first call binds the modules
        feddct_amd.server_aggregate(g, clients)
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        feddct_amd.server_aggregate(g, clients)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    a = getattr(g, "_fa_arena", None)
    sha = hashlib.sha256()     # the result's bits: the same from both trees
    for v in g.state_dict().values():
        sha.update(v.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    rec = {"exp": "tgpu16_ab_dropin", "tree": args.label, "native16": bool(args.native16),
           "native16_master": args.native16 == 2, "master": bool(args.master),
           "layout": args.layout, "dtype": args.dtype, "n": n, "calls": args.calls,
           "bucket_dtype": str(a.f32.dtype) if a is not None else None,
           "staged_keys": len(a._packed) if a is not None else None,
           "global_sha256": sha.hexdigest()[:16],
           "wall_us_median": round(median(ts), 1), "wall_us_min": round(min(ts), 1),
           "wall_us_max": round(max(ts), 1)}
    emit(rec, args.out or os.path.join(
        ROOT, "profiles", "tgpu16_master_dropin.jsonl" if args.master else "tgpu16_dropin.jsonl"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["kernel", "dropin"])
    ap.add_argument("--n", default=None)
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float16"])
    ap.add_argument("--layout", default="wrn16_8_c10")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--native16", type=int, default=1,
                    help="0: option off; 1: native16=True; 2: native16_master=True too")
    ap.add_argument("--master", type=int, default=0, help="1: an fp32 master global")
    ap.add_argument("--tree", default=ROOT, help="checkout whose feddct_amd package is measured")
    ap.add_argument("--label", default="this tree", help="name of --tree in the record")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.n = [int(x) for x in (args.n or ("5,20,32,64" if args.leg == "kernel" else "20")).split(",")]
    sys.path.insert(0, os.path.abspath(args.tree))
    if not torch.cuda.is_available():
        raise SystemExit("tgpu16_ab: no HIP device (a measurement needs the GPU)")
    (kernel_leg if args.leg == "kernel" else dropin_leg)(args)


if __name__ == "__main__":
    main()
