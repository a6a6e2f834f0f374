"""fp16 / bf16 clients reduced into an fp32 master global: the parts that need
no GPU — the C ABI's two new entries and their host-side refusals, the master
layout (the global's fp32 keys at the native 16-bit layout's element offsets)
and arenas bound to CPU modules through both layouts."""
import ctypes

import numpy as np
import pytest
import torch

from feddct_amd import _lib, checkpoint
from feddct_amd.arena import ModuleArena
from feddct_amd.layout import KIND_F32, KIND_H16, KIND_I64, BucketLayout
from helpers import StateModule
from test_abi import header_functions

F32, F16, BF16 = _lib.FA_ELEM_F32, _lib.FA_ELEM_F16, _lib.FA_ELEM_BF16
SHAPES = [1, 7, 8, 31, 33, 100, 2049, 3 * 2048 + 40]


def manifest(dtype):
    keys = [{"key": f"t{j}", "shape": [m], "dtype": dtype} for j, m in enumerate(SHAPES)]
    keys.insert(3, {"key": "nbt", "shape": [], "dtype": "int64"})
    keys.append({"key": "steps", "shape": [5], "dtype": "int64"})
    keys.append({"key": "w", "shape": [3, 5], "dtype": dtype})
    keys.append({"key": "tied", "shape": [33], "dtype": dtype})   # shares t4's slot
    return {"name": "mixed16", "keys": keys}


ALIASES = {"tied": "t4"}


def layout_of(man, **kw):
    return BucketLayout([(e["key"], e["shape"], e["dtype"]) for e in man["keys"]], ALIASES, **kw)


# ------------------------------------------------------------------- ABI ----
def test_new_symbols_are_declared_exported_and_bound():
    new = {"fa_plan_create_elem_out", "fa_plan_out_elem"}
    assert new <= set(header_functions())
    assert new <= set(_lib.EXPORTS)
    for f in new:
        assert getattr(_lib.lib, f).argtypes is not None
    assert len(_lib.lib.fa_plan_create_elem_out.argtypes) == 11
    assert _lib.FA_PLAN_FLAGS_KNOWN == 0x1000000D   # the output type is no flag


def test_host_side_refusals():
    L = _lib.lib
    segs, n = _lib.seg_array(np.array([[0, 4096]], np.int64))
    h = ctypes.c_void_p()

    def create(elem, out_elem, tile=0, flags=1, out=ctypes.byref(h)):
        return L.fa_plan_create_elem_out(segs, n, 4096, None, 0, 0, tile, flags, elem, out_elem,
                                         out)
    legal = {(F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32)}
    for elem in (-1, F32, F16, BF16, 3, 16):
        for out_elem in (-1, F32, F16, BF16, 3, 16):
            if (elem, out_elem) in legal:
                continue
            h.value = 1   # must be cleared or left alone, never a plan
            assert create(elem, out_elem) == _lib.FA_E_INVAL, (elem, out_elem)
            assert b"elem" in L.fa_last_error(), (elem, out_elem)
            assert h.value in (None, 1)
    for elem in (F16, BF16):
        assert create(elem, F32, out=None) == _lib.FA_E_INVAL
        assert b"NULL" in L.fa_last_error()
        assert create(elem, F32, flags=2) == _lib.FA_E_INVAL
        assert b"unknown flag bits" in L.fa_last_error()
        # 16-bit tiles are 2048 or 4096 elements; 1024 is an fp32 width only
        for te in (1024, 3000, 8192):
            assert create(elem, F32, tile=te) == _lib.FA_E_INVAL
            assert b"2048 or 4096" in L.fa_last_error()
    assert L.fa_plan_out_elem(None) == _lib.FA_E_INVAL


@pytest.mark.parametrize("elem", [F32, F16, BF16])
def test_equal_types_is_the_existing_entry(elem):
    """out_elem == elem forwards to fa_plan_create_elem: the same refusals
    with the same messages before any device is touched, and (no device here)
    the table fa_plan_build_host_elem reports for that entry is the only one
    there is — the mixed plan has no table of its own either: the 16-bit
    layout's, whatever the output type."""
    L = _lib.lib
    segs, n = _lib.seg_array(np.array([[0, 10], [5, 10]], np.int64))   # overlapping
    h = ctypes.c_void_p()
    assert L.fa_plan_create_elem(segs, n, 20, None, 0, 0, 0, 0, elem,
                                 ctypes.byref(h)) == _lib.FA_E_INVAL
    want = L.fa_last_error()
    assert L.fa_plan_create_elem_out(segs, n, 20, None, 0, 0, 0, 0, elem, elem,
                                     ctypes.byref(h)) == _lib.FA_E_INVAL
    assert L.fa_last_error() == want and b"overlap" in want
    bad_tile = 8192
    assert L.fa_plan_create_elem(segs, n, 20, None, 0, 0, bad_tile, 0, elem,
                                 ctypes.byref(h)) == _lib.FA_E_INVAL
    want = L.fa_last_error()
    assert L.fa_plan_create_elem_out(segs, n, 20, None, 0, 0, bad_tile, 0, elem, elem,
                                     ctypes.byref(h)) == _lib.FA_E_INVAL
    assert L.fa_last_error() == want
    lay = layout_of(manifest("float32" if elem == F32 else "bfloat16"), native16=elem != F32)
    a = _lib.build_tiles_host(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel, elem=elem)
    assert a[0]["ntiles"] == len(a[1]) > 0


def test_binding_refuses_tiles_and_the_gpu_order_with_an_output_type():
    with pytest.raises(_lib.FedaggError, match="output element type"):
        _lib.Plan(np.array([[0, 4096]]), 4096, elem=BF16, out_elem=F32, tiles=[(0, 2048, 0)])
    with pytest.raises(_lib.FedaggError, match="output element type"):
        _lib.Plan(np.array([[0, 4096]]), 4096, elem=F16, out_elem=F32,
                  order=_lib.FA_ORDER_TORCH_GPU, n=4)
    with pytest.raises(_lib.FedaggError, match="output element type"):
        _lib.Plan(np.array([[0, 4096]]), 4096, elem=F32, out_elem=F32, tiles=[(0, 2048, 0)])


# ---------------------------------------------------------------- layout ----
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_master_layout_has_the_native_16_bit_layouts_offsets(dtype):
    tdt = getattr(torch, dtype)
    master = layout_of(manifest("float32"), master16=True)
    native = layout_of(manifest(dtype), native16=True)
    staged = layout_of(manifest("float32"))
    assert native.native16 and native.float_dtype == tdt
    assert master.master16 and not master.native16 and master.float_dtype == torch.float32
    assert not staged.master16 and not native.master16
    assert master.packed == []
    assert master.keys == native.keys
    for m, h in zip(master.slots, native.slots):
        assert (m.key, m.shape, m.offset, m.numel, m.alias_of) == \
            (h.key, h.shape, h.offset, h.numel, h.alias_of)
        if m.dtype == torch.int64:
            assert m.kind == KIND_I64 == h.kind
        else:
            assert m.dtype == torch.float32 and m.kind == KIND_F32 and h.kind == KIND_H16
            assert m.offset % 128 == 0
    assert master.by_key["tied"].offset == master.by_key["t4"].offset
    assert master.f32_numel == native.f32_numel and master.f32_numel % 128 == 0
    assert master.i64_numel == native.i64_numel == 6
    assert np.array_equal(master.segs32, native.segs32)
    assert np.array_equal(master.segs64, native.segs64)
    assert len({master.signature, native.signature, staged.signature}) == 3
    assert master != staged and master != native
    assert master.f32_numel > staged.f32_numel   # (128- against 64-element boundaries)
    # from a state_dict, with the tie found by storage identity
    mod = StateModule(manifest("float32"))
    mod._parameters["tied"] = mod._parameters["t4"]
    sd = mod.state_dict()   # (parameters first, then buffers)
    got = BucketLayout.from_state_dict(sd, master16=True)
    ent = [(k, tuple(v.shape), v.dtype) for k, v in sd.items()]
    assert got == BucketLayout(ent, ALIASES, master16=True) and got.master16
    assert got.by_key["tied"].alias_of == "t4"
    assert got != BucketLayout.from_state_dict(sd)
    # the master layout is the fp32 global's: no other floating dtype, never both
    with pytest.raises(TypeError, match="t0"):
        layout_of(manifest(dtype), master16=True)
    with pytest.raises(ValueError):
        layout_of(manifest("float32"), native16=True, master16=True)


# ----------------------------------------------------------------- arena ----
def filled(man, seed):
    m = StateModule(man)
    m._parameters["tied"] = m._parameters["t4"]
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for v in m.state_dict().values():
            if v.dtype == torch.int64:
                v.copy_(torch.randint(-50, 50, v.shape, generator=g))
            else:
                v.copy_(torch.randn(v.shape, generator=g))
    return m


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_arenas_bind_global_and_clients_as_views(dtype):
    tdt = getattr(torch, dtype)
    g, c = filled(manifest("float32"), 3), filled(manifest(dtype), 4)
    master = BucketLayout.from_state_dict(g.state_dict(), master16=True)
    native = BucketLayout.from_state_dict(c.state_dict(), native16=True)
    for mod, lay, dt, es in ((g, master, torch.float32, 4), (c, native, tdt, 2)):
        before = {k: v.clone() for k, v in mod.state_dict().items()}
        a = ModuleArena(mod, lay, pinned=False)
        object.__setattr__(mod, "_fa_arena", a)
        assert a._packed == [] and a.f32.dtype == dt and a.f32.numel() == lay.f32_numel
        assert a.extra_keys == []
        lo = a.f32.data_ptr()
        lo64, hi64 = a.i64.data_ptr(), a.i64.data_ptr() + 8 * a.i64.numel()
        for k, v in mod.state_dict().items():
            assert v.dtype == before[k].dtype and torch.equal(v, before[k]), k
            if v.dtype == torch.int64:
                assert lo64 <= v.data_ptr() and v.data_ptr() + 8 * v.numel() <= hi64
            else:
                assert v.data_ptr() == lo + es * lay.by_key[k].offset
        assert a.valid()
    # one set of element offsets under both buckets
    for k in g.state_dict():
        assert master.by_key[k].offset == native.by_key[k].offset
    ck, sd = checkpoint.bucket_state_dict(g), g.state_dict()
    assert list(ck) == list(sd)
    for k in sd:
        assert ck[k].dtype == sd[k].dtype and torch.equal(ck[k], sd[k]), k
        assert ck[k].data_ptr() != sd[k].data_ptr()
