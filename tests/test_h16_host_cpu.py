"""Host-resident fp16 / bf16 rounds in 16-bit buckets: the parts that need no
GPU — the two new C entries (fa_plan_create_from_tiles_elem, fa_narrow_f32)
and their host-side refusals, the cuts partition.py makes of a native 16-bit
layout's tile table, and the layouts the engine picks for host-resident
modules."""
import ctypes

import numpy as np
import pytest
import torch

import hostlayouts as H
from feddct_amd import _lib, aggregate, partition
from feddct_amd.layout import BucketLayout
from feddct_amd.partition import cut_align, i64_tiles, layout_tiles, split_tiles
from helpers import StateModule
from test_abi import header_functions

F32, F16, BF16 = _lib.FA_ELEM_F32, _lib.FA_ELEM_F16, _lib.FA_ELEM_BF16
DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
LEGAL = {(F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32)}


def man16(name, dtype):
    """A hostlayouts manifest with its float dtype replaced."""
    man = H.SWEEP if name == "sweep" else H.LAYOUTS[name]
    return {"keys": [dict(e, dtype=dtype if e["dtype"] == "float32" else e["dtype"])
                     for e in man["keys"]]}


def layout16(name, dtype):
    return BucketLayout([(e["key"], e["shape"], e["dtype"]) for e in man16(name, dtype)["keys"]],
                        native16=True)


def tile_array(tiles):
    arr = (_lib.FaTileDesc * max(1, len(tiles)))()
    for i, (s, c, k) in enumerate(tiles):
        arr[i].start, arr[i].count, arr[i].kind = int(s), int(c), int(k)
    return arr


# ------------------------------------------------------------------- ABI ----
def test_new_symbols_are_declared_exported_and_bound():
    new = {"fa_plan_create_from_tiles_elem", "fa_narrow_f32"}
    assert new <= set(header_functions())
    assert new <= set(_lib.EXPORTS)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for f in new:
        assert hasattr(so, f)
        assert getattr(_lib.lib, f).argtypes is not None
    assert len(_lib.lib.fa_plan_create_from_tiles_elem.argtypes) == 9
    assert len(_lib.lib.fa_narrow_f32.argtypes) == 5
    assert hasattr(_lib.Plan, "from_tiles")


def create(tiles, f32_numel, elem, out_elem, tile=0, flags=1, i64_numel=0, out="h"):
    """(rc, message, handle value) of fa_plan_create_from_tiles_elem.  The
    handle starts as the bogus value 1: a refusal clears it or leaves it
    alone, and never makes a plan (none of these calls reaches a device)."""
    h = ctypes.c_void_p(1)
    rc = _lib.lib.fa_plan_create_from_tiles_elem(
        tile_array(tiles), len(tiles), f32_numel, i64_numel, tile, flags, elem, out_elem,
        ctypes.byref(h) if out == "h" else None)
    return rc, _lib.lib.fa_last_error(), h.value


def test_illegal_element_pairs_are_refused():
    for elem in (-1, F32, F16, BF16, 3, 16):
        for out_elem in (-1, F32, F16, BF16, 3, 16):
            if (elem, out_elem) in LEGAL:
                continue
            rc, msg, h = create([(0, 2048, 0)], 4096, elem, out_elem)
            assert rc == _lib.FA_E_INVAL and b"elem" in msg, (elem, out_elem)
            assert h is None, "*out is cleared first"


@pytest.mark.parametrize("elem,out_elem", sorted(LEGAL - {(F32, F32)}))
def test_host_side_refusals_of_16_bit_tile_subsets(elem, out_elem):
    bad = {
        "start % 8": [(4, 64, 0)],
        "count % 8": [(0, 60, 0)],
        "start % 8 (fp32's 4 is not enough)": [(2044, 8, 0)],
        "count > tile_elems": [(0, 2056, 0)],
        "past the bucket": [(4096 - 8, 16, 0)],
        "scalar tile too long": [(0, 257, 2)],
        "kind": [(0, 8, 7)],
    }
    for what, tiles in bad.items():
        rc, msg, h = create(tiles, 4096, elem, out_elem, tile=2048)
        assert rc == _lib.FA_E_INVAL and b"tile 0" in msg, what
        assert h is None, what
    rc, msg, _ = create([(0, 4096, 0)], 8192, elem, out_elem, tile=2048)
    assert rc == _lib.FA_E_INVAL and b"8-aligned and <= 2048" in msg
    # the 16-bit widths: 2048 and 4096; 1024 is an fp32 width only
    for te in (1024, 3000, 8192):
        rc, msg, h = create([(0, 1024, 0)], 4096, elem, out_elem, tile=te)
        assert rc == _lib.FA_E_INVAL and b"2048 or 4096" in msg and h is None, te
    # overlap: two vector tiles, and a scalar column inside a vector tile
    for tiles in ([(0, 2048, 0), (2040, 64, 0)], [(0, 64, 0), (60, 1, 3)]):
        rc, msg, h = create(tiles, 4096, elem, out_elem)
        assert rc == _lib.FA_E_INVAL and b"overlap" in msg and h is None
    rc, msg, _ = create([(0, 64, 0)], 4096, elem, out_elem, out=None)
    assert rc == _lib.FA_E_INVAL and b"NULL" in msg
    rc, msg, h = create([(0, 64, 0)], 4096, elem, out_elem, flags=2)
    assert rc == _lib.FA_E_INVAL and b"unknown flag bits" in msg and h is None
    n = ctypes.c_void_p(1)
    rc = _lib.lib.fa_plan_create_from_tiles_elem(None, 3, 4096, 0, 0, 1, elem, out_elem,
                                                 ctypes.byref(n))
    assert rc == _lib.FA_E_INVAL and b"bad tile array" in _lib.lib.fa_last_error()
    assert n.value is None


def test_fp32_pair_is_the_existing_entry_with_its_messages():
    L = _lib.lib
    for tiles, f32_numel, tile in ([[(2, 64, 0)], 128, 0], [[(0, 64, 0), (60, 1, 3)], 128, 0],
                                   [[(0, 64, 0)], 128, 3000], [[(0, 64, 0)], 32, 0],
                                   [[(0, 2052, 0)], 4096, 2048]):
        h = ctypes.c_void_p(1)
        assert L.fa_plan_create_from_tiles(tile_array(tiles), len(tiles), f32_numel, 0, tile, 1,
                                           ctypes.byref(h)) == _lib.FA_E_INVAL
        want = L.fa_last_error()
        rc, msg, hv = create(tiles, f32_numel, F32, F32, tile=tile)
        assert rc == _lib.FA_E_INVAL and msg == want and hv is None, tiles
    # (a 4-aligned tile is fine in fp32: it gets past the host checks of both)
    assert b"4-aligned" in create([(2, 64, 0)], 128, F32, F32)[1]
    assert L.fa_plan_create_from_tiles(None, 0, 0, 0, 0, 1, None) == _lib.FA_E_INVAL
    want = L.fa_last_error()
    assert create([], 0, F32, F32, out=None)[1] == want and b"from_tiles: out is NULL" in want


def test_narrow_refusals():
    L = _lib.lib
    buf = (ctypes.c_char * 256)()
    base = (ctypes.addressof(buf) + 15) & ~15
    for elem in (F32, -1, 3):
        assert L.fa_narrow_f32(base, base + 64, elem, 8, None) == _lib.FA_E_INVAL, elem
        assert b"elem" in L.fa_last_error()
    for elem in (F16, BF16):
        assert L.fa_narrow_f32(None, None, elem, 0, None) == _lib.FA_OK
        assert L.fa_narrow_f32(None, base, elem, 8, None) == _lib.FA_E_INVAL
        assert b"NULL" in L.fa_last_error()
        assert L.fa_narrow_f32(base, None, elem, 8, None) == _lib.FA_E_INVAL
        for src, dst in ((base + 4, base + 64), (base, base + 64 + 2), (base + 8, base + 64 + 8)):
            assert L.fa_narrow_f32(src, dst, elem, 8, None) == _lib.FA_E_INVAL
            assert b"aligned" in L.fa_last_error()
        assert L.fa_narrow_f32(base, base + 64, elem, -1, None) == _lib.FA_E_INVAL


def test_plan_binding_keeps_refusing_tiles_in_the_constructor():
    """The tile-subset constructor of other element types is Plan.from_tiles;
    Plan(tiles=...) stays fp32-only."""
    with pytest.raises(_lib.FedaggError, match="no tile subsets"):
        _lib.Plan(np.array([[0, 4096]]), 4096, elem=BF16, tiles=[(0, 2048, 0)])
    with pytest.raises(_lib.FedaggError, match="overlap"):
        _lib.Plan.from_tiles([(0, 64, 0), (60, 1, 3)], 4096, elem=BF16)
    with pytest.raises(_lib.FedaggError, match="out_elem"):
        _lib.Plan.from_tiles([(0, 64, 0)], 4096, elem=F32, out_elem=BF16)


# ------------------------------------------------------------------ cuts ----
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name", ["mid", "noi64", "tiny", "onetile", "sweep"])
def test_cuts_of_16_bit_layouts(name, dtype):
    lay = layout16(name, dtype)
    assert lay.native16 and lay.float_dtype == DTYPES[dtype] and cut_align(lay) == 128
    elem = _lib.ELEM_OF_DTYPE[DTYPES[dtype]]
    info, tiles = layout_tiles(lay)
    want_info, want = _lib.build_tiles_host(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel,
                                            elem=elem)
    assert info == want_info and np.array_equal(tiles, want)
    assert info["tile_elems"] == 2048
    # (the fp32 table of the same segments is another one: vectors of 4)
    t32 = tiles[tiles[:, 2] < 4]
    vec = t32[t32[:, 2] == 0]
    assert np.all(vec[:, 0] % 8 == 0) and np.all(vec[:, 1] % 8 == 0)
    vec_starts = set(vec[:, 0].tolist())
    nonempty = {}
    for cut, (parts, fr) in H.CUTS.items():
        ranges = split_tiles(tiles, parts, lay.f32_numel, fr, cut_align(lay))
        assert len(ranges) == parts
        assert ranges[0][0] == 0 and ranges[-1][1] == lay.f32_numel
        seen = []
        for i, (lo, hi, sel) in enumerate(ranges):
            assert lo <= hi
            if i:
                assert lo == ranges[i - 1][1]
                if lo < lay.f32_numel:   # a real cut: before a vector tile, on 256 B
                    assert lo % 128 == 0 and lo in vec_starts, (cut, lo)
            assert (hi > lo) == (len(sel) > 0), (cut, lo, hi)
            for s, c, _ in sel:
                assert lo <= s and s + c <= hi, "no tile straddles a cut"
            seen += [tuple(t) for t in sel.tolist()]
        assert sorted(seen) == sorted(tuple(t) for t in t32.tolist()), "each tile once"
        nonempty[cut] = sum(hi > lo for lo, hi, _ in ranges)
    if name == "mid":
        assert nonempty["taper"] == 5 and nonempty["taper_nb"] == 2
        assert nonempty["even6"] == 6 and nonempty["even64"] > 6
    if name == "sweep":
        assert nonempty["taper"] == 5 and nonempty["even6"] == 6
    if name in ("tiny", "onetile"):
        assert set(nonempty.values()) == {1}
    assert (len(i64_tiles(tiles)) == 0) == (name == "noi64")


class FakePlan:
    """Records what range_plans asks the library for (no device here)."""
    made = []

    def __init__(self, segs32, f32_numel, segs64=(), i64_numel=0, tile_elems=0, flags=1,
                 tiles=None, **kw):
        assert not kw and segs32 is None and segs64 is None
        FakePlan.made.append(("init", np.asarray(tiles), f32_numel, i64_numel, tile_elems, flags,
                              F32, None))

    @classmethod
    def from_tiles(cls, tiles, f32_numel, i64_numel=0, tile_elems=0, flags=1, elem=F32,
                   out_elem=None):
        cls.made.append(("from_tiles", np.asarray(tiles), f32_numel, i64_numel, tile_elems, flags,
                         elem, out_elem))
        return cls.__new__(cls)


@pytest.fixture
def fake_plans(monkeypatch):
    FakePlan.made = []
    monkeypatch.setattr(_lib, "Plan", FakePlan)
    return FakePlan.made


@pytest.mark.parametrize("name", ["mid", "noi64", "tiny", "onetile", "nof32", "sweep"])
def test_fp32_layouts_get_todays_cuts_and_plans(name, fake_plans):
    man = H.SWEEP if name == "sweep" else H.LAYOUTS[name]
    te = H.SWEEP_TILE if name == "sweep" else 0
    for cut, (parts, fr) in H.CUTS.items():
        lay, tiles, want = H.cut(man, cut, te)
        assert not lay.native16 and cut_align(lay) == 64 and partition.layout_elem(lay) is None
        assert np.array_equal(tiles, _lib.build_tiles_host(lay.segs32, lay.f32_numel, lay.segs64,
                                                           lay.i64_numel, te)[1])
        del fake_plans[:]
        ranges, p64 = partition.range_plans(lay, parts, te, fractions=fr)
        assert [(lo, hi) for lo, hi, _ in ranges] == [(lo, hi) for lo, hi, _ in want]
        assert sum(hi > lo for lo, hi, _ in ranges) == H.NONEMPTY[name][cut]
        made = list(fake_plans)
        assert all(m[0] == "init" for m in made), "fp32 range plans: Plan(tiles=...), as before"
        sels = [sel for _, _, sel in want if len(sel)]
        assert len(made) == len(sels) + (p64 is not None)
        for m, sel in zip(made, sels):
            assert np.array_equal(m[1], sel)
            assert m[2:6] == (lay.f32_numel, lay.i64_numel, te or 2048, 1)
        assert (p64 is None) == (len(i64_tiles(tiles)) == 0)
    with pytest.raises(ValueError):
        partition.range_plans(BucketLayout.from_manifest(H.LAYOUTS["mid"]), 2, out_elem=BF16)


@pytest.mark.parametrize("out_elem", [None, F32])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_range_plans_of_a_16_bit_layout_ask_for_16_bit_or_mixed_plans(dtype, out_elem,
                                                                     fake_plans):
    lay = layout16("mid", dtype)
    elem = _lib.ELEM_OF_DTYPE[DTYPES[dtype]]
    _, tiles = layout_tiles(lay)
    want = split_tiles(tiles, 5, lay.f32_numel, H.TAPER, 128)
    ranges, p64 = partition.range_plans(lay, 5, fractions=H.TAPER, out_elem=out_elem)
    assert [(lo, hi) for lo, hi, _ in ranges] == [(lo, hi) for lo, hi, _ in want]
    assert len(fake_plans) == 6 and p64 is not None
    for m, (_, _, sel) in zip(fake_plans, want):
        assert m[0] == "from_tiles" and np.array_equal(m[1], sel)
        assert m[2:] == (lay.f32_numel, lay.i64_numel, 2048, 1, elem, out_elem)
    assert np.array_equal(fake_plans[-1][1], i64_tiles(tiles))
    assert fake_plans[-1][6:] == (elem, out_elem)


# -------------------------------------------------- the engine's layouts ----
SHAPES = [[], [7], [3, 3], [33], [100], [2049]]


def mod_manifest(dtype, extra=()):
    keys = [{"key": f"t{j}.w", "shape": s, "dtype": dtype} for j, s in enumerate(SHAPES)]
    keys.append({"key": "t.nbt", "shape": [], "dtype": "int64"})
    return {"keys": keys + list(extra)}


def mods(gdtype, cdtype, n=3):
    return StateModule(mod_manifest(gdtype)), [StateModule(mod_manifest(cdtype))
                                               for _ in range(n)]


@pytest.fixture
def eng():
    return aggregate.Engine()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_engine_picks_16_bit_layouts_for_host_resident_sets(eng, dtype):
    tdt = DTYPES[dtype]
    g, cl = mods(dtype, dtype)
    assert eng._round_dtypes(g, cl) == (None, None), "the device qualification is as it was"
    assert eng._host_round_dtypes(g, cl) == ("native", tdt)
    gl, lay = eng.round_layouts(g, cl)
    assert gl is lay and lay.native16 and lay.float_dtype == tdt and not lay.master16
    assert lay.packed == []
    # an fp32 master global
    g, cl = mods("float32", dtype)
    assert eng._round_dtypes(g, cl) == (None, None)
    assert eng._host_round_dtypes(g, cl) == ("mixed", tdt)
    gl, lay = eng.round_layouts(g, cl)
    assert gl is not lay and gl.master16 and gl.float_dtype == torch.float32 and gl.packed == []
    assert lay.native16 and lay.float_dtype == tdt
    assert gl.f32_numel == lay.f32_numel and np.array_equal(gl.segs32, lay.segs32)
    assert np.array_equal(gl.segs64, lay.segs64)
    # whatever the summation order says: a host round takes torch's CPU order
    eng.order = "torch_gpu"
    assert eng._round_dtypes(g, cl) == (None, None)
    assert eng.round_layouts(g, cl)[0].master16
    g, cl = mods(dtype, dtype)
    assert eng.round_layouts(g, cl)[1].native16


def test_engine_keeps_the_fp32_layout_for_every_other_set(eng):
    def staged(g, cl, what):
        assert eng._round_dtypes(g, cl) == (None, None), what
        assert eng._host_round_dtypes(g, cl) == (None, None), what
        gl, lay = eng.round_layouts(g, cl)
        assert gl is lay and not lay.native16 and not lay.master16, what
        assert lay.float_dtype == torch.float32, what

    g, cl = mods("float32", "float32")
    staged(g, cl, "fp32 throughout")
    g, cl = mods("bfloat16", "bfloat16")
    cl[1] = StateModule(mod_manifest("float16"))
    staged(g, cl, "clients of two dtypes")
    g, cl = mods("float32", "bfloat16")
    cl[1] = StateModule(mod_manifest("float16"))
    staged(g, cl, "clients of two dtypes under an fp32 global")
    for gd in ("bfloat16", "float32"):
        g, cl = mods(gd, "bfloat16")
        odd = mod_manifest("bfloat16")
        odd["keys"][3]["dtype"] = "float32"
        cl[2] = StateModule(odd)
        staged(g, cl, "an fp32-keyed client")
    g, cl = mods("float16", "float32")
    staged(g, cl, "a 16-bit global over fp32 clients")
    g, cl = mods("float16", "bfloat16")
    staged(g, cl, "fp16 global over bf16 clients")
    gman = mod_manifest("float32")
    gman["keys"][4]["dtype"] = "bfloat16"
    staged(StateModule(gman), mods("float32", "bfloat16")[1], "a bf16 key in an fp32 global")
    # a module on another device (meta stands in for a GPU here)
    g, cl = mods("bfloat16", "bfloat16")
    staged(g.to("meta"), cl, "a global elsewhere over host clients")
    g, cl = mods("bfloat16", "bfloat16")
    cl[0] = cl[0].to("meta")
    assert eng._host_round_dtypes(g, cl) == (None, None)


def test_an_extra_16_bit_key_in_a_client_still_qualifies(eng):
    """The reference reduces, loads the global and raises in the broadcast:
    the round stays native, the engine's unfused broadcast raises."""
    g, cl = mods("float32", "float16")
    cl[1] = StateModule(mod_manifest("float16", [{"key": "more.w", "shape": [5],
                                                  "dtype": "float16"}]))
    assert eng._host_round_dtypes(g, cl) == ("mixed", torch.float16)
    gl, lay = eng.round_layouts(g, cl)
    assert gl.master16 and lay.native16 and "more.w" not in lay.by_key
