"""The 16-bit proximal term against the fp32 one, one process:
wrn16_8 C100's 50 parameters (2,721 chunks of <= 4096 elements), a client whose
parameters are the global's plus 0.05 randn.

    python tools/prox16_ab.py kernel [--dtype bfloat16] [--rounds 7]
        the forward (partials + finish) and the backward launch of each form
        — fp32 (fa_prox_norms / fa_prox_grad), pure (16-bit global) and mixed
        (fp32 master global) through fa_prox_norms_elem / fa_prox_grad_elem —
        interleaved form by form over several rounds: HIP events around a run
        of back-to-back calls after a warm-up, the buckets rotated through
        sets that together exceed the 256 MB last-level cache several times.
        us (median, min, max over the rounds), GB/s of each launch's own
        algorithmic bytes, the ratio to the fp32 launch of the same elements,
        and the gate: a 16-bit launch is not slower than the fp32 one beyond
        the run-to-run spread the rounds show.
    python tools/prox16_ab.py public [--dtype bfloat16] [--steps 30]
        forward + backward of proximal_term on 16-bit models (both forms,
        per-parameter and one-node) against the reference's own loop on the
        same models in the same process; the gate: the native call is below
        the loop.
    python tools/prox16_ab.py pair [--label NAME]
        the cache policies' A/B: forward then backward on the SAME bucket set,
        back to back, as a training step runs them (the forward's loads decide
        whether the backward finds the buckets in the last-level cache), the
        sets rotated; run it on builds of csrc/prox_h16.hip with other
        -DFA_PROX16_NT_LOAD_FWD / _NT_LOAD_BWD / _NT_STORE settings and name
        each with --label.
    python tools/prox16_ab.py prof [--dtype bfloat16] [--calls 200]
        the three forms' launches back to back, for a kernel trace (run it
        under the profiler; it prints nothing of its own but the plan's size):
        the finish kernels' own times — the pure form's serial 16-bit walk
        over the norms against the fp32 finish — are read from that trace.

Each record is one JSON line, appended to --out (default
profiles/prox16_<leg>.jsonl) and printed.
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


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def models(layout_name, cdt, gdt, dev, seed=1):
    """(client, global): a manifest's keys as a module (BN statistics and
    counters as buffers), the global's parameters 0.05 randn, the client's
    those plus 0.05 randn, cast to the two dtypes."""
    from feddct_amd.layout import BucketLayout
    from feddct_amd.workload import load_manifest
    layout = BucketLayout.from_manifest(load_manifest(layout_name))

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for sl in layout.slots:
                parts = sl.key.split(".")
                mod = self
                for q in parts[:-1]:
                    if q not in mod._modules:
                        mod.add_module(q, torch.nn.Module())
                    mod = mod._modules[q]
                t = torch.zeros(sl.shape, dtype=sl.dtype)
                if sl.dtype == torch.int64 or parts[-1].startswith("running_"):
                    mod.register_buffer(parts[-1], t)
                else:
                    mod.register_parameter(parts[-1], torch.nn.Parameter(t))
    gen = torch.Generator().manual_seed(seed)
    g, c = M(), M()
    with torch.no_grad():
        for pc, pg in zip(c.parameters(), g.parameters()):
            pg.copy_(torch.randn(pg.shape, generator=gen) * 0.05)
            pc.copy_(pg + torch.randn(pg.shape, generator=gen) * 0.05)
    return c.to(cdt).to(dev), g.to(gdt).to(dev)


FORMS = ("f32", "pure", "mixed")


def bound_terms(args, dev):
    """form -> the bound ProximalTerm of a (client, global) pair of that form."""
    from feddct_amd.prox import ProximalTerm
    tdt = getattr(torch, args.dtype)
    dts = {"f32": (torch.float32, torch.float32), "pure": (tdt, tdt), "mixed": (tdt, torch.float32)}
    return {f: ProximalTerm(*models(args.layout, *dts[f], dev)) for f in FORMS}


class Launches:
    """One form's forward and backward over rotating bucket sets."""

    def __init__(self, term, dev, min_bytes=704 << 20):
        from feddct_amd import _lib
        self.L, self.term = _lib.lib, term
        a, b = term.ca.f32, term.ga.f32
        per = 2 * (a.numel() * a.element_size() + b.numel() * b.element_size())
        self.rot = max(4, -(-min_bytes // per))
        self.sets = [(a.clone(), b.clone(), torch.empty_like(a), torch.empty_like(b))
                     for _ in range(self.rot)]
        self.norms = torch.empty(max(1, term.plan.nseg), device=dev)
        tdt = getattr(term, "term_dtype", torch.float32)
        self.total = torch.empty((), device=dev, dtype=tdt)
        self.one = torch.ones((), device=dev, dtype=tdt)
        self.ea = _lib.ELEM_OF_DTYPE[a.dtype]
        self.eb = _lib.ELEM_OF_DTYPE[b.dtype]
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.P = int(sum(m for _, m, _ in term.slots))
        self.esz = (a.element_size(), b.element_size())
        self.check = _lib.check

    def fwd(self, i):
        a, b, _, _ = self.sets[i % self.rot]
        if self.ea == 0:
            rc = self.L.fa_prox_norms(self.term.plan.handle, a.data_ptr(), b.data_ptr(),
                                      self.norms.data_ptr(), self.total.data_ptr(), self.st)
        else:
            rc = self.L.fa_prox_norms_elem(self.term.plan.handle, a.data_ptr(), self.ea,
                                           b.data_ptr(), self.eb, self.norms.data_ptr(),
                                           self.total.data_ptr(), self.st)
        self.check(rc, "forward")

    def bwd(self, i):
        a, b, ga, gb = self.sets[i % self.rot]
        if self.ea == 0:
            rc = self.L.fa_prox_grad(self.term.plan.handle, a.data_ptr(), b.data_ptr(),
                                     self.norms.data_ptr(), self.one.data_ptr(), 1.0,
                                     ga.data_ptr(), gb.data_ptr(), self.st)
        else:
            rc = self.L.fa_prox_grad_elem(self.term.plan.handle, a.data_ptr(), self.ea,
                                          b.data_ptr(), self.eb, self.norms.data_ptr(),
                                          self.one.data_ptr(), 1.0, ga.data_ptr(), gb.data_ptr(),
                                          0, self.st)
        self.check(rc, "backward")

    def bytes(self, leg):
        ea, eb = self.esz
        return self.P * ((ea + eb) if leg == "fwd" else 2 * (ea + eb))


def kernel_leg(args):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    terms = bound_terms(args, dev)
    ls = {f: Launches(terms[f], dev) for f in FORMS}
    for f in FORMS:
        ls[f].fwd(0)     # norms[] for the backward launches
    torch.cuda.synchronize()
    times = {(f, leg): [] for f in FORMS for leg in ("fwd", "bwd")}
    for _ in range(args.rounds):
        for leg in ("fwd", "bwd"):
            for f in FORMS:
                fn = getattr(ls[f], leg)
                reps = args.reps * ls[f].rot
                for i in range(2 * ls[f].rot):
                    fn(i)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(reps):
                    fn(i)
                e1.record()
                e1.synchronize()
                times[(f, leg)].append(e0.elapsed_time(e1) / reps * 1e3)
    rec = {"exp": "prox16_ab_kernel", "layout": args.layout, "dtype": args.dtype,
           "params": ls["f32"].P, "chunks": None, "nseg": terms["f32"].plan.nseg,
           "rounds": args.rounds, "reps_per_set": args.reps,
           "rot": {f: ls[f].rot for f in FORMS}}
    rec["chunks"] = int(sum(-(-m // 4096) for _, m, _ in terms["f32"].slots))
    ok = True
    for leg in ("fwd", "bwd"):
        base = times[("f32", leg)]
        spread = max(max(times[(f, leg)]) - min(times[(f, leg)]) for f in FORMS)
        for f in FORMS:
            t = times[(f, leg)]
            med = median(t)
            r = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                 "bytes": ls[f].bytes(leg), "gbps": round(ls[f].bytes(leg) / med / 1e3, 1),
                 "vs_f32": round(med / median(base), 4)}
            if f != "f32":
                r["not_slower_than_f32"] = bool(med <= median(base) + spread)
                ok = ok and r["not_slower_than_f32"]
            rec[f"{f}_{leg}"] = r
        rec[f"spread_us_{leg}"] = round(spread, 2)
    rec["gate_ok"] = ok
    emit(rec, args.out or os.path.join(ROOT, "profiles", "prox16_kernel.jsonl"))
    return 0 if ok else 1


def public_leg(args):
    from feddct_amd.prox import proximal_term
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    tdt = getattr(torch, args.dtype)
    ok = True
    for form, gdt in (("pure", tdt), ("mixed", torch.float32)):
        client, glob = models(args.layout, tdt, gdt, dev)
        # the reference's loop first, on the unbound models (then on the bound
        # ones: the same tensors, as views of the buckets)

        def reference():
            client.zero_grad(set_to_none=True)
            pt = 0.0
            for w, w_t in zip(client.parameters(), glob.parameters()):
                pt += (w - w_t).norm(2)
            pt.backward()
            return pt

        def ours(flat):
            client.zero_grad(set_to_none=True)
            pt = proximal_term(client, glob, flat_grads=flat)
            pt.backward()
            return pt

        def timed(fn):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) / args.steps * 1e3)
            return ts
        want = float(reference().detach())
        got = float(ours(False).detach())
        t_ref0 = timed(reference)
        t_node = timed(lambda: ours(False))
        t_flat = timed(lambda: ours(True))
        glob.zero_grad(set_to_none=True)
        t_ref1 = timed(reference)
        rec = {"exp": "prox16_ab_public", "layout": args.layout, "dtype": args.dtype, "form": form,
               "steps": args.steps, "rounds": args.rounds, "term_native": got, "term_loop": want,
               "loop_us": round(median(t_ref0), 1), "loop_bound_models_us": round(median(t_ref1), 1),
               "native_us": round(median(t_node), 1), "native_us_max": round(max(t_node), 1),
               "native_flat_grads_us": round(median(t_flat), 1),
               "loop_us_min": round(min(t_ref0 + t_ref1), 1),
               "speedup_vs_loop": round(median(t_ref0) / median(t_node), 2),
               "note": "a step = the client's zero_grad + forward + backward incl. autograd"}
        rec["gate_ok"] = bool(max(t_node) < min(t_ref0 + t_ref1))
        ok = ok and rec["gate_ok"]
        emit(rec, args.out or os.path.join(ROOT, "profiles", "prox16_public.jsonl"))
    return 0 if ok else 1


def pair_leg(args):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    terms = bound_terms(args, dev)
    rec = {"exp": "prox16_ab_pair", "label": args.label, "layout": args.layout,
           "dtype": args.dtype, "rounds": args.rounds, "reps_per_set": args.reps}
    ls = {f: Launches(terms[f], dev) for f in FORMS}
    times = {f: [] for f in FORMS}
    for _ in range(args.rounds):
        for f in FORMS:
            l = ls[f]
            reps = args.reps * l.rot
            for i in range(2 * l.rot):
                l.fwd(i)
                l.bwd(i)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(reps):
                l.fwd(i)
                l.bwd(i)
            e1.record()
            e1.synchronize()
            times[f].append(e0.elapsed_time(e1) / reps * 1e3)
    for f in FORMS:
        t = times[f]
        rec[f] = {"us_median": round(median(t), 2), "us_min": round(min(t), 2),
                  "us_max": round(max(t), 2)}
    emit(rec, args.out or os.path.join(ROOT, "profiles", "prox16_pair.jsonl"))
    return 0


def prof_leg(args):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    terms = bound_terms(args, dev)
    ls = {f: Launches(terms[f], dev) for f in FORMS}
    for i in range(args.calls):
        for f in FORMS:
            ls[f].fwd(i)
            ls[f].bwd(i)
    torch.cuda.synchronize()
    print(json.dumps({"exp": "prox16_ab_prof", "calls": args.calls, "nseg": terms["f32"].plan.nseg}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["kernel", "public", "pair", "prof"])
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float16"])
    ap.add_argument("--layout", default="wrn16_8_c100")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=25, help="kernel leg: calls per bucket set")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--label", default="shipped", help="pair leg: the build's name in the record")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prox16_ab: no HIP device (a measurement needs the GPU)")
    return {"kernel": kernel_leg, "public": public_leg, "pair": pair_leg, "prof": prof_leg}[args.leg](args)


if __name__ == "__main__":
    sys.exit(main())
