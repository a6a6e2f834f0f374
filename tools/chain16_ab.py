"""A chain segment over 16-bit buckets against the fp32 chain segment of the
same rows and the plain 16-bit reduce of the same n, one process, HIP events
(DESIGN §4.15): wrn16_8 C10's vector tiles in bf16 / fp16, clients carved from
one slab, the client sets rotated so that at least 1 GiB is read before a set
repeats, the variants interleaved, median (min - max) of --rounds.

    python tools/chain16_ab.py [--dtype bfloat16,float16] [--cases 20,40,300] [--rounds 7]
                               [--xchg-lib tools/libfedagg_chain16_xchg.so]

--xchg-lib: a second build of libfedagg.so whose fedagg_chain16.hip was
compiled with -DFA_CHAIN16_STATE_XCHG=1 (the state planes through the wide
store's lane exchange instead of adjacent 16-B accesses), loaded beside the
shipped library and timed as the fourth variant, "chain16_xchg"; its state
planes and results are compared bit for bit with the shipped form's.
``--build-xchg`` builds that library (no GPU needed) and exits.

Cases: N = 20 and 40 as a 2-rank split — the first segment (rows 0 .. N/2 - 1,
stores the state) and the last one (loads it, finishes); N = 300, the middle
segment rows 100 .. 199 (two planes in, two out).  Per case and variant: us,
and GB/s of the algorithmic bytes, (n * es + planes_in * 4 + planes_out * 4, or
the result row's es) B per vector-tile element.

Each record is one JSON line, appended to --out (default
profiles/chain16_kernel.jsonl) and printed.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")


def stats(ts, nbytes):
    s = sorted(ts)
    med = s[len(s) // 2]
    return {"us_median": round(med, 2), "us_min": round(s[0], 2), "us_max": round(s[-1], 2),
            "alg_bytes": int(nbytes), "gbps": round(nbytes / med / 1e3, 1)}


def build_xchg(out):
    """libfedagg.so's units, fedagg_chain16.hip with -DFA_CHAIN16_STATE_XCHG=1,
    linked under another soname (the other units' objects are the build's)."""
    import subprocess

    from feddct_amd import build as B
    B.build()
    objdir = os.path.join(B.HERE, "build")
    flags = [f for f in B.FLAGS if f != "-shared"]
    xo = os.path.join(objdir, "fedagg_chain16_xchg.o")
    subprocess.run([B.HIPCC, *flags, "-DFA_CHAIN16_STATE_XCHG=1", "-c", "-o", xo,
                    os.path.join(B.HERE, "csrc", "fedagg_chain16.hip")], check=True)
    objs = [os.path.join(objdir, os.path.basename(s) + ".o") for s in B.SRCS
            if not s.endswith("fedagg_chain16.hip")]
    subprocess.run([B.HIPCC, *B.FLAGS, "-Wl,-soname,libfedagg_chain16_xchg.so", "-o", out, *objs, xo],
                   check=True)
    print(out)


def popc(v):
    return bin(int(v)).count("1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bfloat16,float16")
    ap.add_argument("--cases", default="20,40,300")
    ap.add_argument("--layout", default="wrn16_8_c10")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain16_kernel.jsonl"))
    ap.add_argument("--xchg-lib", default=None)
    ap.add_argument("--build-xchg", action="store_true")
    args = ap.parse_args()
    if args.build_xchg:
        return build_xchg(args.xchg_lib or os.path.join(ROOT, "tools", "libfedagg_chain16_xchg.so"))
    if not torch.cuda.is_available():
        raise SystemExit("chain16_ab: no HIP device (a measurement needs the GPU)")
    from feddct_amd import _lib, slab
    from feddct_amd.layout import BucketLayout
    from feddct_amd.partition import layout_tiles
    from feddct_amd.workload import load_manifest
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = _lib.lib
    X = None
    if args.xchg_lib:
        X = ctypes.CDLL(os.path.abspath(args.xchg_lib))
        for name in ("fa_plan_create_from_tiles_elem", "fa_reduce_chain_elem", "fa_plan_destroy"):
            getattr(X, name).argtypes = getattr(L, name).argtypes
            getattr(X, name).restype = ctypes.c_int
    man = load_manifest(args.layout)
    lay32 = BucketLayout.from_manifest(man)
    _, t32 = layout_tiles(lay32)
    v32 = t32[t32[:, 2] == 0]
    plan32 = _lib.Plan(None, lay32.f32_numel, None, 0, 0, tiles=v32)
    segs = []
    for n in (int(x) for x in args.cases.split(",")):
        if n >= 256:
            segs.append((n, 100, 100, "middle"))
        else:
            segs += [(n, 0, n // 2, "first"), (n, n // 2, n - n // 2, "last")]
    for dtype in args.dtype.split(","):
        tdt = getattr(torch, dtype)
        el = _lib.ELEM_OF_DTYPE[tdt]
        lay16 = BucketLayout([(e["key"], e["shape"], e["dtype"] if e["dtype"] == "int64"
                               else dtype) for e in man["keys"]], native16=True)
        _, t16 = layout_tiles(lay16)
        v16 = t16[t16[:, 2] == 0]
        plan16 = _lib.Plan.from_tiles(v16, lay16.f32_numel, 0, elem=el)
        xplan = ctypes.c_void_p()
        if X is not None:
            arr = (_lib.FaTileDesc * len(v16))()
            for i, (s, c, k) in enumerate(v16):
                arr[i].start, arr[i].count, arr[i].kind = int(s), int(c), int(k)
            assert X.fa_plan_create_from_tiles_elem(arr, len(v16), lay16.f32_numel, 0, 0,
                                                    _lib.FA_PLAN_GAPS_ARE_PADDING, el, el,
                                                    ctypes.byref(xplan)) == 0
        V16, V32 = int(v16[:, 1].sum()), int(v32[:, 1].sum())
        P16 = -(-lay16.f32_numel // 64) * 64
        P32 = -(-lay32.f32_numel // 64) * 64
        for n_total, row0, n, kind in segs:
            lin = L.fa_chain_levels(row0, n_total)
            lout = L.fa_chain_levels(row0 + n, n_total)
            last = row0 + n == n_total
            rot = max(1, -(-(1 << 30) // (n * 2 * lay16.f32_numel)))
            sets = []
            for _ in range(rot):
                slab.release()
                with slab.expecting(2 * n + 2):
                    c32 = [slab.carve(lay32.f32_numel, torch.float32, dev) for _ in range(n)]
                    c16 = [slab.carve(lay16.f32_numel, tdt, dev) for _ in range(n)]
                    o32 = slab.carve(lay32.f32_numel, torch.float32, dev)
                    o16 = slab.carve(lay16.f32_numel, tdt, dev)
                for a, b in zip(c32, c16):
                    a.normal_(0, 0.05)
                    b.normal_(0, 0.05)
                sets.append({"p32": _lib.ptr_array([t.data_ptr() for t in c32]),
                             "p16": _lib.ptr_array([t.data_ptr() for t in c16]),
                             "o32": o32, "o16": o16, "ox": torch.zeros_like(o16),
                             "keep": (c32, c16)})
            # the incoming state: finite values in the planes the levels name
            sin32 = torch.randn(4 * P32, device=dev) * 0.05
            sin16 = torch.randn(4 * P16, device=dev) * 0.05
            sout32, sout16 = torch.zeros_like(sin32), torch.zeros_like(sin16)
            ch32 = _lib.FaChain(row0, n_total, sin32.data_ptr() if lin else None,
                                None if last else sout32.data_ptr(), P32)
            ch16 = _lib.FaChain(row0, n_total, sin16.data_ptr() if lin else None,
                                None if last else sout16.data_ptr(), P16)
            soutx, outx = torch.zeros_like(sin16), None
            ch16x = _lib.FaChain(row0, n_total, sin16.data_ptr() if lin else None,
                                 None if last else soutx.data_ptr(), P16)

            def call(name, i):
                s = sets[i % rot]
                if name == "chain16":
                    rc = L.fa_reduce_chain_elem(plan16.handle, s["p16"], n, None, ctypes.byref(ch16),
                                                s["o16"].data_ptr() if last else None, 0, st)
                elif name == "chain16_xchg":
                    rc = X.fa_reduce_chain_elem(xplan, s["p16"], n, None, ctypes.byref(ch16x),
                                                s["ox"].data_ptr() if last else None, 0, st)
                    assert rc == 0, "chain16_xchg"
                elif name == "chain32":
                    rc = L.fa_reduce_chain(plan32.handle, s["p32"], n, None, ctypes.byref(ch32),
                                           s["o32"].data_ptr() if last else None, 0, st)
                else:
                    rc = L.fa_reduce(plan16.handle, s["p16"], None, n, None, s["o16"].data_ptr(),
                                     None, 0, st)
                _lib.check(rc, name)

            names = ("chain32", "chain16", "reduce16") + (("chain16_xchg",) if X else ())
            reps = max(10, (60 if n > 10 else 120) // max(1, n // 20)) * rot
            times = {k: [] for k in names}
            for _ in range(args.rounds):
                for name in names:
                    for i in range(2 * rot):
                        call(name, i)
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for i in range(reps):
                        call(name, i)
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1) / reps * 1e3)
            pin, pout = popc(lin), (0 if last else popc(lout))
            rec = {"exp": "chain16_ab", "layout": args.layout, "dtype": dtype, "n_total": n_total,
                   "row0": row0, "n": n, "segment": kind, "planes_in": pin, "planes_out": pout,
                   "state_access": "adjacent 16-B", "rot": rot, "reps": reps,
                   "rounds": args.rounds, "vec_elems16": V16, "vec_elems32": V32,
                   "chain32": stats(times["chain32"],
                                    V32 * (n * 4 + pin * 4 + (pout * 4 if pout else 4))),
                   "chain16": stats(times["chain16"],
                                    V16 * (n * 2 + pin * 4 + (pout * 4 if pout else 2))),
                   "reduce16": stats(times["reduce16"], V16 * (n * 2 + 2))}
            if X is not None:
                sout16.zero_()
                call("chain16", 0)
                call("chain16_xchg", 0)
                torch.cuda.synchronize()
                same = torch.equal(sout16.view(torch.int32), soutx.view(torch.int32)) and (
                    not last or torch.equal(sets[0]["o16"].view(torch.int16),
                                            sets[0]["ox"].view(torch.int16)))
                rec["chain16_xchg"] = stats(times["chain16_xchg"], rec["chain16"]["alg_bytes"])
                rec["xchg_same_bits"] = bool(same)
                rec["xchg_vs_adjacent"] = round(rec["chain16_xchg"]["us_median"]
                                                / rec["chain16"]["us_median"], 4)
            c32s = rec["chain32"]
            rec["chain16_vs_chain32"] = round(rec["chain16"]["us_median"] / c32s["us_median"], 4)
            rec["chain32_spread"] = round((c32s["us_max"] - c32s["us_min"]) / c32s["us_median"], 4)
            rec["gate_holds"] = bool(rec["chain16"]["us_median"] <= c32s["us_max"])
            emit(rec, args.out)
            del sets
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
