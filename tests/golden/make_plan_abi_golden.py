"""Cases and goldens of tests/test_plan_refusals_cpu.py and
tests/test_gpu_plan_shape.py: what the eight plan-creating entry points of
libfedagg.so refuse, and the shape of the plans they create.

Both files were recorded from commit 7d941fc, the last one before the
entries were rebuilt over one constructor, with that commit's library:

    python tests/golden/make_plan_abi_golden.py refusals   # no GPU
    python tests/golden/make_plan_abi_golden.py shapes     # on an MI355X

plan_refusals.json: every entry x base (its element types and order) x bad
argument set -> (rc, *out afterwards, fa_last_error()).  A case the recording
library did not refuse before its first device call (FA_E_HIP without a GPU,
or success) is listed under "dropped" instead.  plan_shapes.json: per entry
x variant the plan's fa_plan_info, element types and launch shape / form at
n = 2, 5, 20, unweighted and weighted."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
REFUSALS = os.path.join(HERE, "plan_refusals.json")
SHAPES = os.path.join(HERE, "plan_shapes.json")

F32, F16, BF16 = 0, 1, 2
CPU, GPU = 0, 1
FA_E_HIP = -4
MAX_CLIENTS = 65536
ELEM_NAME = {F32: "f32", F16: "f16", BF16: "bf16"}

# entry -> the arguments it takes besides the layout, flags and out
ENTRIES = {
    "fa_plan_create": ("tile_elems",),
    "fa_plan_create_elem": ("tile_elems", "elem"),
    "fa_plan_create_elem_out": ("tile_elems", "elem", "out_elem"),
    "fa_plan_create_order": ("n", "order"),
    "fa_plan_create_order_elem": ("n", "order", "elem"),
    "fa_plan_create_order_elem_out": ("n", "order", "elem", "out_elem"),
    "fa_plan_create_from_tiles": ("tiles", "tile_elems"),
    "fa_plan_create_from_tiles_elem": ("tiles", "tile_elems", "elem", "out_elem"),
}
GOOD = dict(segs=[[0, 4096]], tiles=[[0, 2048, 0], [2048, 2048, 0]], f32_numel=4096, segs64=[],
            i64_numel=0, tile_elems=0, flags=1, n=4, order=GPU, elem=F32, out_elem=F32, out=True)


def bases(entry):
    """The element types and orders an entry's cases are run under."""
    takes = ENTRIES[entry]
    elems = [{}]
    if "out_elem" in takes:
        elems = [dict(elem=F32, out_elem=F32), dict(elem=F16, out_elem=F16),
                 dict(elem=F16, out_elem=F32)]
    elif "elem" in takes:
        elems = [dict(elem=F32), dict(elem=F16)]
    orders = [dict(order=CPU), dict(order=GPU)] if "order" in takes else [{}]
    out = []
    for e in elems:
        for o in orders:
            b = {**e, **o}
            name = "/".join(([ELEM_NAME[b["elem"]]] if "elem" in b else []) +
                            (["out_" + ELEM_NAME[b["out_elem"]]] if "out_elem" in b else []) +
                            ([("cpu", "gpu")[b["order"]]] if "order" in b else [])) or "-"
            out.append((name, b))
    return out


SINGLES = {
    "null_out": dict(out=False),
    "flag40": dict(flags=0x41),
    "neg_size": dict(f32_numel=-1),
    "neg_i64": dict(i64_numel=-1),
    "tile3000": dict(tile_elems=3000),
    "elem9": dict(elem=9),
    "f32_out_bf16": dict(elem=F32, out_elem=BF16),
    "f16_out_bf16": dict(elem=F16, out_elem=BF16),
    "order5": dict(order=5),
    "n1": dict(n=1),
    "n_max1": dict(n=MAX_CLIENTS + 1),
    "overlap": dict(segs=[[0, 10], [5, 10]], tiles=[[0, 2048, 0], [1024, 2048, 0]]),
    "past_end": dict(segs=[[0, 5000]], tiles=[[0, 2048, 0], [4000, 2048, 0]]),
    "misaligned16": dict(segs=[[4, 2048]], tiles=[[4, 2048, 0]]),
    "n512": dict(n=512, segs=[[0, 1024]], f32_numel=1024),
}
PAIRS = [
    ("null_out", "flag40"), ("null_out", "order5"), ("null_out", "elem9"),
    ("null_out", "f16_out_bf16"), ("null_out", "f32_out_bf16"), ("null_out", "neg_size"),
    ("flag40", "order5"), ("flag40", "neg_size"), ("flag40", "f16_out_bf16"),
    ("flag40", "f32_out_bf16"), ("flag40", "elem9"), ("flag40", "tile3000"), ("flag40", "n512"),
    ("flag40", "misaligned16"), ("order5", "n1"), ("order5", "elem9"), ("order5", "overlap"),
    ("order5", "f32_out_bf16"), ("order5", "f16_out_bf16"), ("n1", "elem9"), ("n1", "overlap"),
    ("n1", "past_end"), ("n1", "f16_out_bf16"), ("n_max1", "neg_size"), ("elem9", "overlap"),
    ("elem9", "tile3000"), ("elem9", "neg_size"), ("neg_size", "tile3000"),
    ("neg_size", "overlap"), ("tile3000", "overlap"), ("tile3000", "f16_out_bf16"),
    ("neg_i64", "past_end"), ("f16_out_bf16", "overlap"),
]
CASES = dict(SINGLES)
for _a, _b in PAIRS:
    assert not set(SINGLES[_a]) & set(SINGLES[_b]), (_a, _b)
    CASES[_a + "+" + _b] = {**SINGLES[_a], **SINGLES[_b]}


def applies(entry, case):
    """A case applies to an entry that takes every argument it sets."""
    own = set(ENTRIES[entry]) | {"out", "flags", "f32_numel", "i64_numel", "segs", "tiles"}
    return all(k in own for k in CASES[case])


def enumerate_cases():
    return [(e, bn, c) for e in ENTRIES for bn, _ in bases(e) for c in CASES if applies(e, c)]


def _segs(L, rows):
    from feddct_amd import _lib
    arr = (_lib.FaSeg * max(1, len(rows)))()
    for i, (o, m) in enumerate(rows):
        arr[i].offset, arr[i].numel = o, m
    return arr, len(rows)


def call(entry, args):
    """Call `entry` with GOOD overridden by `args`: (rc, handle value after the
    call from a sentinel of 1, message)."""
    from feddct_amd import _lib
    L = _lib.lib
    a = {**GOOD, **args}
    takes = ENTRIES[entry]
    h = ctypes.c_void_p(1)
    if "tiles" in takes:
        arr = (_lib.FaTileDesc * max(1, len(a["tiles"])))()
        for i, (s, c, k) in enumerate(a["tiles"]):
            arr[i].start, arr[i].count, arr[i].kind = s, c, k
        argv = [arr, len(a["tiles"]), a["f32_numel"], a["i64_numel"]]
    else:
        argv = [*_segs(L, a["segs"]), a["f32_numel"], *_segs(L, a["segs64"]), a["i64_numel"]]
    argv += [a[k] for k in ("tile_elems", "n", "order") if k in takes]
    argv.append(a["flags"])
    argv += [a[k] for k in ("elem", "out_elem") if k in takes]
    argv.append(ctypes.byref(h) if a["out"] else None)
    rc = getattr(L, entry)(*argv)
    msg = L.fa_last_error().decode() if rc else ""
    return rc, h.value or 0, msg


def run_case(entry, base, case):
    return call(entry, {**dict(bases(entry))[base], **CASES[case]})


def record_refusals():
    rows, dropped = [], []
    for e, b, c in enumerate_cases():
        rc, h, msg = run_case(e, b, c)
        if rc == 0 or rc == FA_E_HIP:
            if rc == 0:
                from feddct_amd import _lib
                _lib.lib.fa_plan_destroy(ctypes.c_void_p(h))
            dropped.append([e, b, c])
        else:
            rows.append([e, b, c, rc, h, msg])
    return {"parent": "7d941fc", "rows": rows, "dropped": dropped}


# ------------------------------------------------------------- shapes ----
# One layout with every tile kind: a tensor of two full fp32 tiles (one full
# 16-bit tile), a partial vector tile and a 3-element tail, a lone scalar, a
# tensor that starts off a vector boundary, and a 3-element int64 segment.
SHAPE_SEGS = [[0, 5155], [5155, 1], [5157, 40]]
SHAPE_NUMEL = 5248
SHAPE_SEGS64 = [[0, 3]]
SHAPE_NUMEL64 = 3
SHAPE_N = (2, 5, 20)
ELEM_PAIRS = [(F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32)]


def shape_variants():
    """(entry, variant name, arguments) of every plan the shape test creates."""
    out = []
    orders = [("cpu", dict(order=CPU, n=0))] + [(f"gpu{n}", dict(order=GPU, n=n)) for n in SHAPE_N]
    for entry, takes in ENTRIES.items():
        if "out_elem" in takes:
            elems = [(f"{ELEM_NAME[e]}/out_{ELEM_NAME[o]}", dict(elem=e, out_elem=o))
                     for e, o in ELEM_PAIRS]
        elif "elem" in takes:
            elems = [(ELEM_NAME[e], dict(elem=e)) for e in (F32, F16, BF16)]
        else:
            elems = [("f32", {})]
        for en, ea in elems:
            for on, oa in (orders if "order" in takes else [("cpu", {})]):
                out.append((entry, f"{en}/{on}", {**ea, **oa}))
    return out


def shape_args(entry, args):
    from feddct_amd import _lib
    a = dict(segs=SHAPE_SEGS, f32_numel=SHAPE_NUMEL, segs64=SHAPE_SEGS64, i64_numel=SHAPE_NUMEL64,
             **args)
    if "tiles" in ENTRIES[entry]:
        elem = args.get("elem", F32)
        _, tiles = _lib.build_tiles_host(SHAPE_SEGS, SHAPE_NUMEL, SHAPE_SEGS64, SHAPE_NUMEL64,
                                         elem=None if elem == F32 else elem)
        a["tiles"] = [[int(x) for x in t] for t in tiles]
    return a


def shape_record(entry, args):
    """What the tests compare of the plan `entry` creates with `args`."""
    from feddct_amd import _lib
    L = _lib.lib
    rc, h, msg = call(entry, shape_args(entry, args))
    if rc:
        return {"rc": rc, "message": msg}
    h = ctypes.c_void_p(h)
    try:
        info = _lib.FaPlanInfo()
        _lib.check(L.fa_plan_get_info(h, ctypes.byref(info)), "fa_plan_get_info")
        rec = {"rc": 0, "info": {f: getattr(info, f) for f, _ in _lib.FaPlanInfo._fields_},
               "elem": L.fa_plan_elem(h), "out_elem": L.fa_plan_out_elem(h), "launch": {}}
        for n in SHAPE_N:
            for w in (0, 1):
                v = [ctypes.c_int() for _ in range(5)]
                _lib.check(L.fa_plan_launch_shape(h, n, w, ctypes.byref(v[0]), ctypes.byref(v[1])),
                           "fa_plan_launch_shape")
                _lib.check(L.fa_plan_launch_form(h, n, w, ctypes.byref(v[2]), ctypes.byref(v[3]),
                                                 ctypes.byref(v[4])), "fa_plan_launch_form")
                rec["launch"][f"n{n}/w{w}"] = [x.value for x in v]
        return rec
    finally:
        _lib.check(L.fa_plan_destroy(h), "fa_plan_destroy")


def record_shapes():
    return {"parent": "7d941fc",
            "plans": {f"{e}:{v}": shape_record(e, a) for e, v, a in shape_variants()}}


def dump(obj, path, key):
    """JSON with one row of obj[key] per line."""
    rows = obj[key]
    items = rows.items() if isinstance(rows, dict) else None
    with open(path, "w") as f:
        f.write("{")
        for k, v in obj.items():
            if k != key:
                f.write(f"{json.dumps(k)}: {json.dumps(v)},\n")
        if items is None:
            f.write(f"{json.dumps(key)}: [\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]}\n")
        else:
            f.write(f"{json.dumps(key)}: {{\n" +
                    ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in items) + "\n}}\n")


if __name__ == "__main__":
    out = sys.argv[2] if len(sys.argv) > 2 else None
    if sys.argv[1] == "refusals":
        dump(record_refusals(), out or REFUSALS, "rows")
    else:
        dump(record_shapes(), out or SHAPES, "plans")
