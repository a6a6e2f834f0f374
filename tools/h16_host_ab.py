"""Host-resident fp16 / bf16 rounds: wall time of one
``server_aggregate`` call, broadcast included, with the global and the N
clients in host memory — wrn16_8 C10's shapes (10,972,154 elements per model),
N = 20 plus the global.  The public call only, so the same script measures
another checkout of the package (``--tree``): run it on this tree and on the
parent commit, alternating, two runs each.

    python tools/h16_host_ab.py [--tree DIR] [--label NAME] [--case bf16,mixed,fp32]
                                [--n 20] [--calls 10] [--warmup 2] [--out FILE]

cases   bf16 / fp16   every model cast to the 16-bit dtype
        mixed         an fp32 global over bf16 clients (mixed16: over fp16)
        fp32          fp32 host modules: the yardstick on the same tree

Per case one JSON line (appended to --out, default
profiles/h16_host_round.jsonl, and printed): median, min and max of --calls
calls after --warmup, the layout kind the arenas were bound with (native16 /
master16 / fp32: which path ran), the bytes one client's floating keys put on
PCIe per direction, and the implied GB/s of the round's algorithmic bytes,
(N + 1) x the clients' state bytes (2 B per element in the 16-bit cases).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {"bf16": ("bfloat16", "bfloat16"), "fp16": ("float16", "float16"),
         "mixed": ("float32", "bfloat16"), "mixed16": ("float32", "float16"),
         "fp32": ("float32", "float32")}


class StateModule(torch.nn.Module):
    """A module whose state_dict has exactly a manifest's keys."""

    def __init__(self, manifest, dtype, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        for e in manifest["keys"]:
            parts = e["key"].split(".")
            mod = self
            for p in parts[:-1]:
                if p not in mod._modules:
                    mod.add_module(p, torch.nn.Module())
                mod = mod._modules[p]
            if e["dtype"] == "int64":
                mod.register_buffer(parts[-1], torch.randint(0, 500, e["shape"], generator=g))
            else:
                t = (torch.randn(e["shape"], generator=g) * 0.05).to(getattr(torch, dtype))
                mod.register_parameter(parts[-1], torch.nn.Parameter(t))


def kind_of(module):
    lay = module._fa_arena.layout
    return "native16" if lay.native16 else "master16" if getattr(lay, "master16", False) \
        else "fp32"


def run_case(case, args, feddct_amd, manifest):
    gd, cd = CASES[case]
    g = StateModule(manifest, gd, 999)
    clients = [StateModule(manifest, cd, i) for i in range(args.n)]
    elems = sum(v.numel() for v in clients[0].state_dict().values() if v.dtype != torch.int64)
    i64 = sum(v.numel() for v in clients[0].state_dict().values() if v.dtype == torch.int64)
    es = 4 if cd == "float32" else 2
    ts = []
    for k in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        feddct_amd.server_aggregate(g, clients)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if k >= args.warmup:
            ts.append(dt * 1e3)
    ts.sort()
    med = ts[len(ts) // 2]
    alg = (args.n + 1) * (es * elems + 8 * i64)
    return {"tool": "h16_host_ab", "label": args.label, "case": case, "n": args.n,
            "global": gd, "clients": cd, "elems": elems, "calls": args.calls,
            "warmup": args.warmup, "ms_median": round(med, 3), "ms_min": round(ts[0], 3),
            "ms_max": round(ts[-1], 3), "global_layout": kind_of(g),
            "client_layout": kind_of(clients[0]),
            "bucket_dtype": str(clients[0]._fa_arena.f32.dtype).replace("torch.", ""),
            "staged_keys_per_client": len(clients[0]._fa_arena._packed),
            "upload_bytes": args.n * clients[0]._fa_arena.f32.element_size() * elems,
            "algorithmic_bytes": alg, "algorithmic_gbps": round(alg / (med * 1e-3) / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="checkout whose feddct_amd is measured")
    ap.add_argument("--label", default="this")
    ap.add_argument("--case", default="bf16,mixed,fp32")
    ap.add_argument("--layout", default="wrn16_8_c10")
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "h16_host_round.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import feddct_amd
    from feddct_amd.workload import load_manifest
    assert os.path.abspath(feddct_amd.__file__).startswith(os.path.abspath(args.tree))
    manifest = load_manifest(args.layout)
    torch.cuda.set_device(0)
    for case in args.case.split(","):
        rec = run_case(case, args, feddct_amd, manifest)
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        from feddct_amd import aggregate
        aggregate._ENGINE = None      # the next case binds its own buckets and pipeline


if __name__ == "__main__":
    main()
