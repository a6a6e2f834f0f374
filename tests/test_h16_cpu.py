"""fp16 / bf16 model state reduced natively from 16-bit buckets: the parts
that need no GPU — the C ABI's new entries and their host-side refusals, the
host tile table of a 16-bit layout, the native layout, and arenas bound to
CPU modules."""
import ctypes

import numpy as np
import pytest
import torch

from feddct_amd import _lib, checkpoint
from feddct_amd.arena import ModuleArena
from feddct_amd.layout import KIND_H16, KIND_I64, KIND_PACKF, BucketLayout
from helpers import StateModule
from test_abi import KIND_NAME, _expected_kind, header_functions

ELEMS = {"float16": 1, "bfloat16": 2}
SHAPES = [1, 7, 8, 31, 32, 33, 100, 2048, 2049, 3 * 2048 + 40]


def manifest(dtype, odd=None):
    keys = [{"key": f"t{j}", "shape": [m], "dtype": dtype} for j, m in enumerate(SHAPES)]
    keys.insert(3, {"key": "nbt", "shape": [], "dtype": "int64"})
    keys.append({"key": "steps", "shape": [5], "dtype": "int64"})
    keys.append({"key": "w", "shape": [3, 5], "dtype": dtype})
    if odd is not None:
        keys[odd[0]]["dtype"] = odd[1]
    return {"name": "h16", "keys": keys}


def layout_of(man, **kw):
    return BucketLayout([(e["key"], e["shape"], e["dtype"]) for e in man["keys"]], **kw)


# ------------------------------------------------------------------- ABI ----
def test_new_symbols_are_declared_exported_and_bound():
    new = {"fa_plan_create_elem", "fa_plan_build_host_elem", "fa_plan_elem"}
    assert new <= set(header_functions())
    assert new <= set(_lib.EXPORTS)
    for f in new:
        assert getattr(_lib.lib, f).argtypes is not None
    assert (_lib.FA_ELEM_F32, _lib.FA_ELEM_F16, _lib.FA_ELEM_BF16) == (0, 1, 2)
    assert _lib.FA_PLAN_FLAGS_KNOWN == 0x1000000D   # the element type is no flag


def test_host_side_refusals():
    L = _lib.lib
    segs, n = _lib.seg_array(np.array([[0, 4096]], np.int64))
    info = _lib.FaPlanInfo()
    h = ctypes.c_void_p()
    for bad in (-1, 3, 16):
        assert L.fa_plan_build_host_elem(segs, n, 4096, None, 0, 0, 0, 1, bad, None, 0,
                                         ctypes.byref(info)) == _lib.FA_E_INVAL
        assert b"elem" in L.fa_last_error()
        assert L.fa_plan_create_elem(segs, n, 4096, None, 0, 0, 0, 1, bad,
                                     ctypes.byref(h)) == _lib.FA_E_INVAL
        assert b"elem" in L.fa_last_error()
    for elem in (1, 2):
        # 16-bit tiles are 2048 or 4096 elements; 1024 is an fp32 width only
        for te in (1024, 3000, 8192):
            assert L.fa_plan_build_host_elem(segs, n, 4096, None, 0, 0, te, 1, elem, None, 0,
                                             ctypes.byref(info)) == _lib.FA_E_INVAL
            assert b"2048 or 4096" in L.fa_last_error()
            assert L.fa_plan_create_elem(segs, n, 4096, None, 0, 0, te, 1, elem,
                                         ctypes.byref(h)) == _lib.FA_E_INVAL
        assert L.fa_plan_build_host_elem(segs, n, 4096, None, 0, 0, 0, 2, elem, None, 0,
                                         ctypes.byref(info)) == _lib.FA_E_INVAL
        assert b"unknown flag bits" in L.fa_last_error()
        assert L.fa_plan_create_elem(segs, n, 4096, None, 0, 0, 0, 1, elem,
                                     None) == _lib.FA_E_INVAL
        assert L.fa_plan_build_host_elem(segs, n, 4096, None, 0, 0, 0, 1, elem, None, 0,
                                         None) == _lib.FA_E_INVAL
        assert L.fa_plan_build_host_elem(segs, n, 100, None, 0, 0, 0, 1, elem, None, 0,
                                         ctypes.byref(info)) == _lib.FA_E_INVAL  # outside bucket
    assert L.fa_plan_elem(None) == _lib.FA_E_INVAL
    # tile subsets and the torch-GPU order make fp32 plans only: the binding
    # refuses before any library call
    with pytest.raises(_lib.FedaggError, match="16-bit"):
        _lib.Plan(np.array([[0, 4096]]), 4096, elem=_lib.FA_ELEM_BF16, tiles=[(0, 2048, 0)])
    with pytest.raises(_lib.FedaggError, match="16-bit"):
        _lib.Plan(np.array([[0, 4096]]), 4096, elem=_lib.FA_ELEM_F16,
                  order=_lib.FA_ORDER_TORCH_GPU, n=4)


# ----------------------------------------------------------- host tiles ----
@pytest.mark.parametrize("dtype", sorted(ELEMS))
@pytest.mark.parametrize("tile", [0, 2048, 4096])
def test_host_tile_table_of_a_16_bit_layout(dtype, tile):
    lay = layout_of(manifest(dtype), native16=True)
    assert lay.native16
    info, tiles = _lib.build_tiles_host(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel,
                                        tile, flags=0, elem=ELEMS[dtype])
    assert info["ntiles"] == len(tiles)
    width = info["tile_elems"]
    assert width == (tile or width) and width in (2048, 4096)
    cover16 = np.zeros(lay.f32_numel, np.int64)
    cover64 = np.zeros(lay.i64_numel, np.int64)
    kind16 = np.full(lay.f32_numel, "", dtype=object)
    kind64 = np.full(lay.i64_numel, "", dtype=object)
    for start, count, kind in tiles:
        assert 1 <= count <= (width if kind == 0 else 256)
        cov, kd = (cover64, kind64) if kind >= 4 else (cover16, kind16)
        cov[start:start + count] += 1
        kd[start:start + count] = KIND_NAME[kind]
        if kind == 0:   # 16-B vectors of 8 elements
            assert start % 8 == 0 and count % 8 == 0, (start, count)
    want16 = np.zeros(lay.f32_numel, np.int64)
    for o, M in lay.segs32:
        want16[o:o + M] = 1
        for col in range(M):
            assert kind16[o + col] == _expected_kind(M, col), (o, M, col)
    for o, M in lay.segs64:
        for col in range(M):
            assert kind64[o + col] == _expected_kind(M, col)
    assert np.array_equal(cover16, want16), "every element of a key exactly once, no gap covered"
    assert (cover64 == 1).all()
    assert info["cascade_elems"] + info["tail_elems"] == int(lay.segs32[:, 1].sum())
    # with the gaps declared padding the vector runs may span them; still
    # every key element exactly once, in its order
    info2, tiles2 = _lib.build_tiles_host(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel,
                                          tile, elem=ELEMS[dtype])
    cover = np.zeros(lay.f32_numel, np.int64)
    for start, count, kind in tiles2:
        if kind < 4:
            cover[start:start + count] += 1
            assert kind != 0 or (start % 8 == 0 and count % 8 == 0)
    assert cover.max() == 1 and (cover[want16 == 1] == 1).all()


@pytest.mark.parametrize("tile", [0, 1024, 2048, 4096])
def test_fp32_element_type_is_the_existing_table(tile):
    lay = layout_of(manifest("float32"))
    a = _lib.build_tiles_host(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel, tile)
    b = _lib.build_tiles_host(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel, tile,
                              elem=_lib.FA_ELEM_F32)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


def test_unaligned_and_short_cascade_bodies_go_scalar():
    """A 16-bit vector is 8 elements: a key at an offset that is no multiple
    of 8, and the 4-column body of a 4..7-element key, keep the cascade order
    one column per thread."""
    segs = np.array([[0, 64], [68, 64], [136, 6], [256, 64]], np.int64)
    _, tiles = _lib.build_tiles_host(segs, 320, flags=0, elem=_lib.FA_ELEM_BF16)
    got = sorted((int(s), int(c), int(k)) for s, c, k in tiles)
    assert got == [(0, 64, 0), (68, 64, 1), (136, 4, 1), (140, 2, 2), (256, 64, 0)]


# ---------------------------------------------------------------- layout ----
@pytest.mark.parametrize("dtype", sorted(ELEMS))
def test_native_layout_of_a_homogeneous_16_bit_state(dtype):
    man = manifest(dtype)
    tdt = getattr(torch, dtype)
    lay = layout_of(man, native16=True)
    assert lay.native16 and lay.float_dtype == tdt and lay.packed == []
    for s in lay.slots:
        if s.dtype == torch.int64:
            assert s.kind == KIND_I64
        else:
            assert s.kind == KIND_H16 and s.offset % 128 == 0
    assert lay.f32_numel % 128 == 0
    nel = sum(int(np.prod(e["shape"])) for e in man["keys"] if e["dtype"] != "int64")
    assert lay.state_bytes() == 2 * nel + 8 * 6
    # the default is today's staged layout, and a different layout object
    old = layout_of(man)
    assert not old.native16 and old.float_dtype == torch.float32
    assert all(s.kind == KIND_PACKF for s in old.slots if s.dtype != torch.int64)
    assert all(s.offset % 64 == 0 for s in old.slots if s.kind == KIND_PACKF)
    assert old.state_bytes() == 4 * nel + 8 * 6
    assert old != lay and old.signature != lay.signature
    sd = StateModule(man).state_dict()   # (parameters first, then buffers)
    ent = [(k, tuple(v.shape), v.dtype) for k, v in sd.items()]
    got = BucketLayout.from_state_dict(sd, native16=True)
    assert got == BucketLayout(ent, native16=True) and got.native16
    assert {s.kind for s in got.slots} == {KIND_H16, KIND_I64}
    assert BucketLayout.from_state_dict(sd) == BucketLayout(ent)
    assert not BucketLayout.from_state_dict(sd).native16


@pytest.mark.parametrize("odd", ["float32", "float16", "float64", "int32"])
def test_mixed_state_keeps_the_staged_layout(odd):
    man = manifest("bfloat16", odd=(5, odd))
    lay = layout_of(man, native16=True)
    assert lay == layout_of(man) and not lay.native16
    assert KIND_H16 not in {s.kind for s in lay.slots}
    f32 = layout_of(manifest("float32"), native16=True)
    assert not f32.native16 and f32 == layout_of(manifest("float32"))


# ----------------------------------------------------------------- arena ----
def filled(man, seed):
    m = StateModule(man)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for v in m.state_dict().values():
            if v.dtype == torch.int64:
                v.copy_(torch.randint(-50, 50, v.shape, generator=g))
            else:
                v.copy_(torch.randn(v.shape, generator=g))
    return m


@pytest.mark.parametrize("dtype", sorted(ELEMS))
def test_arena_binds_16_bit_cpu_modules_as_views(dtype):
    man = manifest(dtype)
    tdt = getattr(torch, dtype)
    m = filled(man, 3)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    lay = BucketLayout.from_state_dict(m.state_dict(), native16=True)
    a = ModuleArena(m, lay, pinned=False)
    object.__setattr__(m, "_fa_arena", a)
    assert a._packed == [] and a.f32.dtype == tdt and a.f32.numel() == lay.f32_numel
    lo, hi = a.f32.data_ptr(), a.f32.data_ptr() + 2 * a.f32.numel()
    lo64, hi64 = a.i64.data_ptr(), a.i64.data_ptr() + 8 * a.i64.numel()
    for k, v in m.state_dict().items():
        assert v.dtype == before[k].dtype and torch.equal(v, before[k]), k
        if v.dtype == torch.int64:
            assert lo64 <= v.data_ptr() and v.data_ptr() + 8 * v.numel() <= hi64
        else:
            s = lay.by_key[k]
            assert v.data_ptr() == lo + 2 * s.offset and v.data_ptr() + 2 * v.numel() <= hi
    assert a.valid()
    ck = checkpoint.bucket_state_dict(m)
    sd = m.state_dict()
    assert list(ck) == list(sd)
    for k in sd:
        assert ck[k].dtype == sd[k].dtype and ck[k].shape == sd[k].shape
        assert torch.equal(ck[k], sd[k]), k
        assert ck[k].data_ptr() != sd[k].data_ptr()


def test_arena_refuses_a_module_whose_key_dtype_differs():
    man = manifest("bfloat16")
    lay = layout_of(man, native16=True)
    with pytest.raises(TypeError, match="t4"):
        ModuleArena(filled(manifest("bfloat16", odd=(5, "float32")), 1), lay, pinned=False)
    with pytest.raises(TypeError):
        ModuleArena(filled(manifest("float16"), 1), lay, pinned=False)
