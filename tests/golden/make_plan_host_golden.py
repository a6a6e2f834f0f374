"""Cases and goldens of tests/test_plan_host_cpu.py.

The goldens (plan_host_digests.json: per case the SHA-256 of the raw tables
and the tile count) were recorded from commit 88975e2, the last one whose
planners lived inside csrc/fedagg.hip, NOT from plan_host.cpp:

    git worktree add /tmp/parent 88975e2
    python tests/golden/make_plan_host_golden.py /tmp/parent

which patches the parent's csrc/fedagg.hip (PATCH below: the HIP allocation
calls of plan creation become malloc / memcpy and the two occupancy queries
return forced slot counts, so plan creation runs without a device; three
debug exports dump a plan's tables and a call's launch choice), builds it,
creates every case's plan through the parent's public entry points and
hashes what the plan holds.  The blob layout is the one
tests/host/plan_host_check.cpp writes.

The case list is part of the JSON (the refused torch-GPU-order configuration
is found by scanning with the parent), and the test reads it from there."""
import ctypes
import hashlib
import json
import os
import struct
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PARENT = "88975e2"
OUT = os.path.join(HERE, "plan_host_digests.json")

# (anchor line of the parent's fedagg.hip, text inserted after it)
PATCH = [
    ('#include "h16.h"\n', """
static int g_s8 = 0, g_s16 = 0, g_tg = 0;
#define hipGetDevice(d) (*(d) = 0, hipSuccess)
#define hipMalloc(p, n) (*(void**)(p) = malloc(n), hipSuccess)
#define hipMemcpy(d, s, n, k) (memcpy(d, s, n), hipSuccess)
#define hipFree(p) (free(p), hipSuccess)
"""),
    ("int kernel_slots(int dev, int u, int b, bool deep, bool w) {\n",
     "  if (true) return b == 16 ? g_s16 : g_s8;\n"),
    ("int tgpu_slots(int dev, int batch) {\n", "  if (true) return g_tg;\n"),
    (None, """
extern "C" void fa_dbg_slots(int s8, int s16, int tg) { g_s8 = s8; g_s16 = s16; g_tg = tg; }
extern "C" int fa_dbg_dump(const fa_plan* p, const char* path) {
  FILE* f = fopen(path, "wb");
  if (!f) return -1;
  auto i32 = [&](int32_t v) { fwrite(&v, 4, 1, f); };
  auto i64 = [&](int64_t v) { fwrite(&v, 8, 1, f); };
  if (p->order == FA_ORDER_TORCH_GPU) {
    for (int g = 0; g < 6; ++g) i32(p->tg_lo[g]);
    i32(p->info.ntiles);
    if (p->info.ntiles) fwrite(p->d_tiles, sizeof(Tile), p->info.ntiles, f);
    if (p->info.ntiles) fwrite(p->d_fac, 4, p->info.ntiles, f);
  } else {
    fwrite(&p->info, sizeof p->info, 1, f);
    i32(p->flat_bcast); i32(p->vec_u); i32(p->nt_dev); i32(p->ns_dev);
    i32(p->nt_alt_dev); i32(p->ns_alt_dev); i64(p->sidx_alt_off);
    const int64_t ns = (int64_t)(p->ns_dev + p->ns_alt_dev) * kPackCols;
    i64(ns);
    if (p->nt_dev) fwrite(p->d_tiles, sizeof(Tile), p->nt_dev, f);
    if (p->nt_alt_dev) fwrite(p->d_tiles_alt, sizeof(Tile), p->nt_alt_dev, f);
    if (ns) fwrite(p->d_sidx, 8, ns, f);
    i32((int32_t)p->bal.size());
    for (const fa_plan::BalTable& b : p->bal) {
      i32(b.u); i32(b.slots); i32(b.batch); i32(b.alt); i32(b.nt);
      fwrite(b.d, sizeof(Tile), b.nt, f);
    }
  }
  fclose(f);
  return 0;
}
extern "C" void fa_dbg_launch(const fa_plan* p, int n, int w, int32_t* row) {
  const Launch L = select_launch(p, n, w != 0, 0);
  int table = L.tiles == p->d_tiles ? -1 : L.tiles == p->d_tiles_alt ? -2 : -3;
  for (size_t i = 0; i < p->bal.size(); ++i)
    if (L.tiles == p->bal[i].d) table = (int)i;
  const int r[7] = {table, L.nt, L.ns, L.vec_u, L.batch, L.slots, pipe_rule(p, L, n, w != 0)};
  for (int i = 0; i < 7; ++i) row[i] = r[i];
}
"""),
]

GAPS = 1                 # FA_PLAN_GAPS_ARE_PADDING
LAUNCH_N = (1, 2, 7, 8, 11, 12, 16, 17, 63, 64, 128, 129, 200, 255, 256, 300)
TGPU_N = (2, 5, 9, 10, 20, 32, 48, 64, 100, 127, 128, 300)
SLOT_TABLES = ((0, 0), (1280, 768), (1024, 1024))   # (8-client, 16-client kernels)

# One synthetic layout of edge shapes: five adjacent one-element fp32 keys and
# three adjacent one-element int64 keys (four fit a torch-GPU-order tile, one
# wave each), keys of 2, 3, 5, 31, 33 and 2049 elements, a 2049-element key at
# an offset that is no multiple of 4 (head, body and tail), an empty segment,
# and a gap of 104 elements.
EDGE = {"f32_numel": 8448, "i64_numel": 8,
        "seg32": [[0, 1], [1, 1], [2, 1], [3, 1], [4, 1], [5, 2], [8, 3], [12, 5], [20, 31],
                  [52, 33], [87, 2049], [2136, 0], [2240, 4096], [6336, 2049]],
        "seg64": [[0, 1], [1, 1], [2, 1], [3, 5]]}


def load_layouts():
    """name -> {f32_numel, i64_numel, seg32, seg64} (lists of [offset, numel])."""
    sys.path.insert(0, ROOT)
    from feddct_amd.layout import BucketLayout
    out = {"edge": EDGE}
    for name, path in (("small", os.path.join(HERE, "small_manifest.json")),
                       ("wrn16_8_c10", None), ("resnet110sl_sf4_c100_main", None)):
        path = path or os.path.join(ROOT, "feddct_amd", "manifests", name + ".json")
        with open(path) as f:
            man = json.load(f)
        lay = BucketLayout.from_manifest(man.get("small", man))   # small_manifest.json holds several
        out[name] = {"f32_numel": int(lay.f32_numel), "i64_numel": int(lay.i64_numel),
                     "seg32": lay.segs32.tolist(), "seg64": lay.segs64.tolist()}
    return out


def cases(refused_n):
    out = []
    for lay in ("small", "wrn16_8_c10", "resnet110sl_sf4_c100_main", "edge"):
        for flags in (0, GAPS):
            for te in (1024, 2048, 0):
                for s8, s16 in SLOT_TABLES:
                    out.append({"name": f"{lay}/default/te{te}/f{flags}/s{s8}-{s16}",
                                "kind": "default", "layout": lay, "tile_elems": te,
                                "flags": flags, "elem": 0, "s8": s8, "s16": s16})
            for te in (2048, 4096):
                out.append({"name": f"{lay}/h16/te{te}/f{flags}", "kind": "default",
                            "layout": lay, "tile_elems": te, "flags": flags, "elem": 1,
                            "s8": 0, "s16": 0})
            for n in TGPU_N + ((refused_n,) if lay == "edge" else ()):
                for slots in (0, 768, 1280):
                    out.append({"name": f"{lay}/tgpu/n{n}/f{flags}/s{slots}", "kind": "tgpu",
                                "layout": lay, "n": n, "flags": flags, "slots": slots})
    return out


def case_file(cs, layouts):
    """The text tests/host/plan_host_check.cpp reads."""
    lines = []
    for name in sorted({c["layout"] for c in cs}):
        L = layouts[name]
        lines.append(f"layout {name} {L['f32_numel']} {L['i64_numel']} {len(L['seg32'])} "
                     f"{len(L['seg64'])}")
        lines += [f"{o} {m}" for o, m in L["seg32"] + L["seg64"]]
    for c in cs:
        if c["kind"] == "default":
            lines.append(f"default {c['name']} {c['layout']} {c['tile_elems']} {c['flags']} "
                         f"{c['elem']} {c['s8']} {c['s16']}")
        else:
            lines.append(f"tgpu {c['name']} {c['layout']} {c['n']} {c['flags']} {c['slots']}")
    return "\n".join(lines) + "\n"


def read_records(path):
    """name -> blob of a plan_host_check output file."""
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


def ntiles(kind, blob):
    """The (main) table's tile count of a case's blob; None for a refusal."""
    if kind == "default":
        return struct.unpack_from("<i", blob, 48 + 8)[0]
    return struct.unpack_from("<i", blob, 28)[0] if struct.unpack_from("<i", blob)[0] == 0 else None


# ------------------------------------------------------- the parent's side --
def _patched_parent(parent):
    src = os.path.join(parent, "feddct_amd", "csrc", "fedagg.hip")
    with open(src) as f:
        text = f.read()
    if "fa_dbg_dump" not in text:
        for anchor, ins in PATCH:
            if anchor is None:
                text += ins
            else:
                assert text.count(anchor) == 1, anchor
                text = text.replace(anchor, anchor + ins)
        with open(src, "w") as f:
            f.write(text)
    subprocess.run([sys.executable, "-c", "from feddct_amd import build as b; b.build()"],
                   cwd=parent, check=True)
    return ctypes.CDLL(os.path.join(parent, "feddct_amd", "libfedagg.so"))


def _segs(rows):
    arr = (ctypes.c_int64 * (2 * len(rows)))(*[v for r in rows for v in r])
    return arr, len(rows)


def main(parent):
    lib = _patched_parent(parent)
    lib.fa_torch_gpu_config.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_void_p]
    layouts = load_layouts()
    refused_n = next(n for n in range(2, 4097)
                     if any(m and not lib.fa_torch_gpu_config(n, m, None)
                            for _, m in EDGE["seg32"] + EDGE["seg64"]))
    tmp = os.path.join(parent, "plan_dump.bin")
    done = []
    for c in cases(refused_n):
        L = layouts[c["layout"]]
        s32, n32 = _segs(L["seg32"])
        s64, n64 = _segs(L["seg64"])
        plan = ctypes.c_void_p()
        args = (s32, n32, ctypes.c_int64(L["f32_numel"]), s64, n64, ctypes.c_int64(L["i64_numel"]))
        blobs = {}
        if c["kind"] == "default":
            lib.fa_dbg_slots(c["s8"], c["s16"], 0)
            rc = lib.fa_plan_create_elem(*args, c["tile_elems"], c["flags"], c["elem"],
                                         ctypes.byref(plan))
            assert rc == 0, (c, rc)
            assert lib.fa_dbg_dump(plan, tmp.encode()) == 0
            with open(tmp, "rb") as f:
                blobs[c["name"]] = f.read()
            if c["elem"] == 0:
                rows = b""
                for n in LAUNCH_N:
                    for w in (0, 1):
                        row = (ctypes.c_int32 * 7)()
                        lib.fa_dbg_launch(plan, n, w, row)
                        rows += bytes(row)
                blobs[c["name"] + "/launch"] = rows
        else:
            lib.fa_dbg_slots(0, 0, c["slots"])
            rc = lib.fa_plan_create_order(*args, c["n"], 1, c["flags"], ctypes.byref(plan))
            blob = struct.pack("<i", rc)
            if rc == 0:
                assert lib.fa_dbg_dump(plan, tmp.encode()) == 0
                with open(tmp, "rb") as f:
                    blob += f.read()
            blobs[c["name"]] = blob
        if plan:
            lib.fa_plan_destroy(plan)
        d = dict(c)
        d["sha256"] = hashlib.sha256(blobs[c["name"]]).hexdigest()
        d["ntiles"] = ntiles(c["kind"], blobs[c["name"]])
        if c["name"] + "/launch" in blobs:
            d["launch_sha256"] = hashlib.sha256(blobs[c["name"] + "/launch"]).hexdigest()
        done.append(d)
    os.remove(tmp)
    with open(OUT, "w") as f:
        json.dump({"parent": PARENT, "cases": done}, f, indent=0)
        f.write("\n")
    print(len(done), "cases ->", OUT)


if __name__ == "__main__":
    main(sys.argv[1])
