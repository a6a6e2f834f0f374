"""Cases and goldens of tests/test_sched_host_cpu.py.

The goldens (sched_host_digests.json: per case the SHA-256 of every rank's
raw fa_xfer list and of the fa_round_cost bytes, plus the op count; per
selection case the SHA-256 of (mode, nchunks, model_us)) were recorded from
commit 875cce3, the last one whose schedules and cost model lived inside
csrc/fedcomm.hip, NOT from sched_host.cpp:

    git worktree add /tmp/parent 875cce3
    (cd /tmp/parent && python -m feddct_amd.build)
    python tests/golden/make_sched_host_golden.py /tmp/parent/feddct_amd/libfedagg_comm.so

which imports the feddct_amd package that library belongs to and records,
through its comm.describe / comm.round_model / comm.multi_select, the bytes
tests/host/sched_host_check.cpp writes.  No FA_MODEL_* variable may be set.

The JSON lists the cases by name, in cases()'s order; the test compares the
names with cases() and takes each case's parameters from there."""
import hashlib
import json
import os
import re
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PARENT = "875cce3"
OUT = os.path.join(HERE, "sched_host_digests.json")

SHARDED, STRIPED, CHAINED, BLOCKED = 0, 1, 2, 3
MODE_NAMES = {SHARDED: "e1", STRIPED: "striped", CHAINED: "chained", BLOCKED: "blocked"}
REASSOCIATE, ROOT_ALL = 1, 2        # FA_MULTI_*
FA_E_INVAL, FA_E_RANGE = -1, -2

# tests/test_schedule.py's MAN: ten fp32 keys (empty, 1-element and
# non-multiple-of-4 ones among them) and two int64 keys
_F32 = [100, 4096, 33, 2048 + 8, 7, 0, 5000, 1, 64, 3000]
MAN = {"keys": [{"key": f"k{j}", "shape": [m] if m else [], "dtype": "float32"}
                for j, m in enumerate(_F32)]
       + [{"key": "nbt", "shape": [], "dtype": "int64"},
          {"key": "nbt2", "shape": [], "dtype": "int64"}]}
NOI64 = {"keys": MAN["keys"][:len(_F32)]}
# fa_multi_select's nominal layout: one fp32 tensor of 2^24 elements
NOMINAL = {"keys": [{"key": "w", "shape": [1 << 24], "dtype": "float32"}]}
# tests/test_schedule.py's COUNTS (world sizes 2-8, empty and uneven shards), and one rank
COUNTS = [[10, 10], [7, 0, 13], [3, 3, 3, 3, 3, 3, 3, 3], [0, 5, 1, 14], [4, 9, 0, 2, 5],
          [1, 1, 1, 17], [16, 16, 1], [2, 30, 2, 0, 0, 1, 3, 2], [9]]
# tests/test_multi_default.py test_select_named_shapes' count shapes
SELECT_COUNTS = [[3] * 8, [20] * 8, [10, 10], [7, 0, 13], [1, 1, 1, 17]]


def load_layouts():
    """name -> {f32_numel, i64_numel, seg32, seg64} (lists of [offset, numel])."""
    sys.path.insert(0, ROOT)
    from feddct_amd.layout import BucketLayout
    with open(os.path.join(ROOT, "feddct_amd", "manifests", "wrnsl16_8_sf4_c100_main.json")) as f:
        wrnsl = json.load(f)
    out = {}
    for name, man in (("man", MAN), ("noi64", NOI64), ("wrnsl", wrnsl), ("nominal", NOMINAL)):
        lay = BucketLayout.from_manifest(man)
        out[name] = {"f32_numel": int(lay.f32_numel), "i64_numel": int(lay.i64_numel),
                     "seg32": lay.segs32.tolist(), "seg64": lay.segs64.tolist()}
    return out


def _rounds(layout, counts_list, combos):
    """Every mode (e1 with both exchanges) of every count vector under each
    (root, weighted, nchunks) of `combos`."""
    out = []
    for counts in counts_list:
        W = len(counts)
        for mode in (SHARDED, STRIPED, CHAINED, BLOCKED):
            for xchg in ((0, 1) if mode == SHARDED else (0,)):
                for root, weighted, k in combos:
                    root = {"last": W - 1, "beyond": W}.get(root, root)
                    cs = "-".join(map(str, counts))
                    out.append({"name": f"{layout}/{MODE_NAMES[mode]}/c{cs}/r{root}/"
                                        f"w{weighted}/k{k}/x{xchg}",
                                "kind": "round", "layout": layout, "counts": counts,
                                "mode": mode, "nchunks": k, "xchg": xchg, "root": root,
                                "weighted": weighted})
    return out


# (root, weighted, nchunks): every root kind with and without weights, every
# chunk count; what a builder branches on beside the counts and the mode is
# the root kind (one rank / every rank; chained: the finisher or not), the
# weights (e1's division, e2's staging) and the chunk count, independently
COMBOS = [(0, 0, 5), (-1, 1, 0), ("last", 0, 1), ("last", 1, 5), (-1, 0, 1)]


def cases():
    out = _rounds("man", COUNTS, COMBOS)
    out += _rounds("man", COUNTS[:1], [("beyond", 0, 5)])            # refused: root >= nranks
    out += _rounds("noi64", [[10, 10], [0, 5, 1, 14], [9]], COMBOS[:2])
    out += _rounds("wrnsl", [[3] * 8], [(-1, 0, 0), ("last", 1, 5)])   # the cfg5 shape
    assert len({c["name"] for c in out}) == len(out)
    for layout, flags in (("man", (0, ROOT_ALL, REASSOCIATE)), ("wrnsl", (0, ROOT_ALL)),
                          ("nominal", (0, ROOT_ALL))):
        for counts in SELECT_COUNTS:
            for mflags in flags:
                cs = "-".join(map(str, counts))
                out.append({"name": f"{layout}/select/c{cs}/m{mflags}", "kind": "select",
                            "layout": layout, "counts": counts, "mflags": mflags})
    return out


def blocked_allowed(counts):
    """Every cascade block of 16 slots (below 65,536 slots in all) lies on at
    most two of the ranks holding slots: feddct_amd.dist.blocked_allowed."""
    sys.path.insert(0, ROOT)
    from feddct_amd.dist import blocked_allowed as f
    return f(counts)


def expected_refusal(c):
    """The return code a round case must be refused with, or 0."""
    if c["root"] >= len(c["counts"]):
        return FA_E_INVAL
    if c["mode"] == BLOCKED and not blocked_allowed(c["counts"]):
        return FA_E_RANGE
    return 0


def case_file(cs, layouts):
    """The text tests/host/sched_host_check.cpp reads."""
    lines = []
    for name in sorted({c["layout"] for c in cs}):
        L = layouts[name]
        lines.append(f"layout {name} {L['f32_numel']} {L['i64_numel']} {len(L['seg32'])} "
                     f"{len(L['seg64'])}")
        lines += [f"{o} {m}" for o, m in L["seg32"] + L["seg64"]]
    for c in cs:
        tail = f"{len(c['counts'])} " + " ".join(map(str, c["counts"]))
        if c["kind"] == "round":
            lines.append(f"round {c['name']} {c['layout']} {c['mode']} {c['nchunks']} {c['xchg']} "
                         f"{c['root']} {c['weighted']} {tail}")
        else:
            lines.append(f"select {c['name']} {c['layout']} {c['mflags']} {tail}")
    return "\n".join(lines) + "\n"


def read_records(path):
    """name -> blob of a sched_host_check output file."""
    with open(path, "rb") as f:
        data = f.read()
    out, pos = {}, 0
    while pos < len(data):
        (nl,) = struct.unpack_from("<i", data, pos)
        name = data[pos + 4:pos + 4 + nl].decode()
        (bl,) = struct.unpack_from("<q", data, pos + 4 + nl)
        pos += 12 + nl
        out[name] = data[pos:pos + bl]
        pos += bl
    return out


XFER = "<8i2q2i"         # fa_xfer: 56 B, no padding
COST = "<3d2i"           # fa_round_cost


def round_rcs(blob, nranks):
    """(per-rank return codes, ops in all) of a round case's schedule blob."""
    rcs, nops, pos = [], 0, 0
    for _ in range(nranks):
        (rc,) = struct.unpack_from("<i", blob, pos)
        pos += 4
        rcs.append(rc)
        if rc == 0:
            (n,) = struct.unpack_from("<i", blob, pos)
            pos += 4 + 56 * n
            nops += n
    assert pos == len(blob)
    return rcs, nops


# ------------------------------------------------------- the parent's side --
def _rc_of(err):
    return int(re.search(r"failed \((-?\d+)\)", str(err)).group(1))


def main(libpath):
    libpath = os.path.realpath(libpath)
    parent = os.path.dirname(os.path.dirname(libpath))
    assert not [v for v in os.environ if v.startswith("FA_MODEL_")], "unset FA_MODEL_*"
    layouts = load_layouts()          # (the segment lists, from this tree's manifests)
    for m in [m for m in sys.modules if m == "feddct_amd" or m.startswith("feddct_amd.")]:
        del sys.modules[m]
    sys.path.insert(0, parent)
    from feddct_amd import _lib
    from feddct_amd import comm as C
    from feddct_amd.layout import BucketLayout
    assert os.path.realpath(C.COMM_PATH) == libpath, (C.COMM_PATH, libpath)
    with open(os.path.join(ROOT, "feddct_amd", "manifests", "wrnsl16_8_sf4_c100_main.json")) as f:
        wrnsl = json.load(f)
    lay = {n: BucketLayout.from_manifest(m) for n, m in
           (("man", MAN), ("noi64", NOI64), ("wrnsl", wrnsl), ("nominal", NOMINAL))}
    for n, L in lay.items():
        assert L.segs32.tolist() == layouts[n]["seg32"] and L.segs64.tolist() == layouts[n]["seg64"]
    done = []
    for c in cases():
        # (the name spells every parameter out: the JSON keeps it and the digests)
        L, counts, d = lay[c["layout"]], c["counts"], {"name": c["name"]}
        if c["kind"] == "select":
            name, k, us = C.multi_select(counts, exact=not c["mflags"] & REASSOCIATE, layout=L,
                                         root_all=bool(c["mflags"] & ROOT_ALL), detail=True)
            blob = struct.pack("<iiid", 0, C.MODE_IDS[name], k, us)
            d["sha256"] = hashlib.sha256(blob).hexdigest()
            done.append(d)
            continue
        kw = dict(nchunks=c["nchunks"], exchange=c["xchg"], root=c["root"],
                  weighted=bool(c["weighted"]))
        blob = b""
        for r in range(len(counts)):
            try:
                ops = C.describe(c["mode"], L, counts, r, **kw)
            except _lib.FedaggError as e:
                blob += struct.pack("<i", _rc_of(e))
                continue
            blob += struct.pack("<ii", 0, len(ops))
            for x in ops:
                blob += struct.pack(XFER, x["step"], C.X[x["op"]], x["peer"], x["chunk"],
                                    C.B[x["src"]], x["src_index"], C.B[x["dst"]], x["dst_index"],
                                    x["offset"], x["count"], x["row0"], x["nrows"])
        try:
            m = C.round_model(c["mode"], L, counts, **kw)
            model = struct.pack("<i", 0) + struct.pack(
                COST, m["model_us"], m["link_bytes_max"], m["hbm_bytes_max"], m["groups"],
                m["steps"])
        except _lib.FedaggError as e:
            model = struct.pack("<i", _rc_of(e))
        rcs, nops = round_rcs(blob, len(counts))
        d["sha256"] = hashlib.sha256(blob).hexdigest()
        d["model_sha256"] = hashlib.sha256(model).hexdigest()
        d["nops"] = nops if not any(rcs) else None
        done.append(d)
    with open(OUT, "w") as f:   # one case per line
        rows = ",\n".join(json.dumps(d, separators=(",", ":")) for d in done)
        f.write('{"parent":"%s","cases":[\n%s\n]}\n' % (PARENT, rows))
    print(len(done), "cases ->", OUT)


if __name__ == "__main__":
    main(sys.argv[1])
