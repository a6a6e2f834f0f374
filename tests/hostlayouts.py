"""Layouts of the host-resident round's tests (test_gpu_host_round.py) and the
cuts pipeline.HostPipeline makes of them, pinned on a CPU by
test_partition.py: a GPU test that depends on a cut's shape asserts it, so a
change of the planner cannot quietly turn it into a one-chunk test."""
from feddct_amd.layout import BucketLayout
from feddct_amd.partition import layout_tiles, split_tiles

TAPER = (0.5, 0.25, 0.125, 0.0625, 0.0625)            # HostPipeline.TAPER
TAPER_NO_BCAST = (0.9375, 0.0625)                     # HostPipeline.TAPER_NO_BCAST


def manifest(f32_shapes, n_i64):
    keys = [{"key": f"k{j}", "shape": list(sh), "dtype": "float32"}
            for j, sh in enumerate(f32_shapes)]
    keys += [{"key": f"nbt{j}", "shape": [], "dtype": "int64"} for j in range(n_i64)]
    return {"keys": keys}


LAYOUTS = {
    "mid": manifest([[7], [64, 64, 3, 3], [], [4097], [128, 64, 3, 3], [2049], [33], [16384],
                     [5]], 2),
    "tiny": manifest([[3], []], 1),
    "onetile": manifest([[2048]], 1),
    "noi64": manifest([[4097], [100]], 0),
    "nof32": manifest([], 2),
}

# the client-count sweep's layout, cut at tile_elems=1024: unaligned key
# lengths and scalar tails, 42 tiles, 36 KiB of fp32 per client
SWEEP = manifest([[5], [4097], [], [1023], [9000], [33], [2049], [16385], [3], [1025], [7000],
                  [100], [2]], 2)
SWEEP_TILE = 1024

# cut name -> (parts, fractions)
CUTS = {"taper": (len(TAPER), TAPER), "taper_nb": (len(TAPER_NO_BCAST), TAPER_NO_BCAST),
        "even6": (6, None), "even64": (64, None)}

# non-empty ranges of each cut of each layout
NONEMPTY = {
    "mid": {"taper": 5, "taper_nb": 2, "even6": 6, "even64": 64},
    "tiny": {"taper": 1, "taper_nb": 1, "even6": 1, "even64": 1},
    "onetile": {"taper": 1, "taper_nb": 1, "even6": 1, "even64": 1},
    "noi64": {"taper": 2, "taper_nb": 2, "even6": 3, "even64": 3},
    "nof32": {"taper": 0, "taper_nb": 0, "even6": 0, "even64": 0},
    "sweep": {"taper": 5, "taper_nb": 2, "even6": 6, "even64": 42},
}
MID_TAPER_SIZES = [67593, 32768, 16385, 8225, 8197]


def cut(man, name, tile_elems=0):
    """(layout, tiles, [(lo, hi, tiles in range)]) of the named cut."""
    layout = BucketLayout.from_manifest(man)
    _, tiles = layout_tiles(layout, tile_elems)
    parts, fr = CUTS[name]
    return layout, tiles, split_tiles(tiles, parts, layout.f32_numel, fr)
