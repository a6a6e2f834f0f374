"""The torch-GPU-order planner for 16-bit buckets (plan_host.cpp plan_tgpu
with 8-element vectors) without a GPU, through the library's host entry
fa_plan_build_order_host_elem: every table is checked for coverage, vector
alignment, the row split and factor of every key, and its launch groups
(tgpu16cases.check_table); the fp32 element type gives the fp32 planner's
table; the refusals of the entry and of the binding hold.  The stand-alone
program tests/host/tgpu16_host_check.cpp runs the same entry over the same
kinds of layout from plain C++ (it is the one to build with sanitizers)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tgpu16cases as C
from conftest import ROOT
from feddct_amd import _lib

L = _lib.lib


def build(segs32, numel32, segs64, numel64, n, flags, elem, slots=0):
    return _lib.build_order_tiles_host(segs32, numel32, segs64, numel64, n=n, flags=flags,
                                       elem=elem, slots=slots)


def test_new_symbols_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "fedagg.h")).read()
    for f in ("fa_plan_create_order_elem", "fa_plan_build_order_host_elem"):
        assert f + "(" in src and f in _lib.EXPORTS and hasattr(L, f)
    assert hasattr(_lib.Plan, "for_order")


@pytest.mark.parametrize("n", C.PLAN_NS)
@pytest.mark.parametrize("dtype", sorted(C.ELEMS))
def test_tables_of_native_16_bit_layouts(dtype, n):
    # keys torch splits across blocks at this N are outside the restatement
    sizes = tuple(m for m in C.KEY_SIZES if C.config(n, m)[0])
    assert len(sizes) >= len(C.KEY_SIZES) - 5
    lay = C.manifest_layout(dtype, sizes)
    for flags in (0, C.GAPS):
        for slots in (0, 8):
            tiles, fac, lo = build(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel, n, flags,
                                   C.ELEMS[dtype], slots)
            C.check_table(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel, n, flags,
                          C.ELEMS[dtype], tiles, fac, lo)
    # full 2048-element vector tiles exist, and the int64 key has its tile
    assert any(c == 2048 and (k & 0xFF) in (C.K_V, C.K_W) for _, c, k in tiles)
    assert sum((k & 0xFF) == C.K_INNER64 for _, _, k in tiles) == 1


@pytest.mark.parametrize("flags", [0, C.GAPS])
@pytest.mark.parametrize("n", C.PLAN_NS)
@pytest.mark.parametrize("dtype", sorted(C.ELEMS))
def test_tables_of_raw_segment_lists(dtype, n, flags):
    segs, numel = C.raw_segments(n)
    assert {int(o) % 8 for o, _ in segs} == set(range(8))
    s64 = np.array([[0, 1], [3, 36]], np.int64)
    tiles, fac, lo = build(segs, numel, s64, 40, n, flags, C.ELEMS[dtype])
    C.check_table(segs, numel, s64, 40, n, flags, C.ELEMS[dtype], tiles, fac, lo)
    # the head of a key that starts off a 16-B boundary is one scalar tile of
    # (8 - offset % 8) % 8 elements, and its body starts on the boundary
    scal = {(int(s), int(c)) for s, c, k in tiles if (k & 0xFF) == C.K_SCALAR}
    vtiles = [(int(s), int(c)) for s, c, k in tiles if (k & 0xFF) in (C.K_V, C.K_W)]
    for o, m in segs:
        o, m = int(o), int(m)
        head = min((8 - o % 8) % 8, m)
        if m > 1 and head:
            assert (o, head) in scal, (o, m)
        if m > 1 and (m - head) >= 8:
            assert any(s <= o + head < s + c for s, c in vtiles), (o, m)


def test_aligned_keys_share_one_run_and_padding_joins_across_a_gap():
    """(128, 256, 4096) back to back are one run of 4,480 elements: two full
    tiles and one of 384; the 512-element key 16 elements on joins it only
    when the gaps are declared padding."""
    segs, numel = C.raw_segments()
    first = int(segs[32, 0])
    assert [int(m) for _, m in segs[32:35]] == [128, 256, 4096] and first % 8 == 0
    for flags, want in ((0, [2048, 2048, 384]), (C.GAPS, [2048, 2048, 912])):
        tiles, _, _ = build(segs, numel, (), 0, 5, flags, _lib.FA_ELEM_BF16)
        run = sorted((int(s), int(c)) for s, c, k in tiles
                     if (k & 0xFF) == C.K_W and first <= s < first + 4480 + 16 + 512)
        assert [c for _, c in run][:3] == want, (flags, run)


@pytest.mark.parametrize("n", [2, 17, 64, 256])
def test_fp32_element_type_is_the_fp32_table(n):
    """elem = FA_ELEM_F32 through the new entry: 4-element vectors, S >= 4
    tiles of 1,024 elements — the fp32 planner's table (the stand-alone
    program compares it with plan_tgpu's, tile by tile)."""
    sizes = tuple(m for m in C.KEY_SIZES if C.config(n, m)[0])
    from feddct_amd.layout import BucketLayout
    ent = [(f"t{j}", (m,) if m > 1 else (), "float32") for j, m in enumerate(sizes)]
    lay = BucketLayout(ent + [("nbt", (), "int64")])
    tiles, fac, lo = build(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel, n, C.GAPS,
                           _lib.FA_ELEM_F32)
    C.check_table(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel, n, C.GAPS,
                  _lib.FA_ELEM_F32, tiles, fac, lo)
    assert all(s % 4 == 0 for s, _, k in tiles if (k & 0xFF) in (C.K_V, C.K_W))


def _rc(segs, numel, n, elem, flags=0, order=_lib.FA_ORDER_TORCH_GPU, slots=0):
    a32, n32 = _lib.seg_array(np.asarray(segs, np.int64))
    import ctypes
    nt = ctypes.c_int(-1)
    rc = L.fa_plan_build_order_host_elem(a32, n32, numel, None, 0, 0, n, order, flags, elem, slots,
                                         None, None, 0, None, ctypes.byref(nt))
    return rc, L.fa_last_error().decode()


def test_host_entry_refusals():
    segs = [[0, 1024]]
    bf = _lib.FA_ELEM_BF16
    assert _rc(segs, 1024, 2, bf)[0] == _lib.FA_OK
    for n in (-1, 0, 1, _lib.FA_MAX_CLIENTS + 1):
        rc, msg = _rc(segs, 1024, n, bf)
        assert rc == _lib.FA_E_RANGE and "outside 2.." in msg, (n, rc, msg)
    rc, msg = _rc(segs, 1024, 4, 7)
    assert rc == _lib.FA_E_INVAL and "elem must be" in msg
    rc, msg = _rc(segs, 1024, 4, bf, flags=0x40)
    assert rc == _lib.FA_E_INVAL and "unknown flag bits" in msg
    rc, msg = _rc(segs, 1024, 4, bf, order=_lib.FA_ORDER_TORCH_CPU)
    assert rc == _lib.FA_E_INVAL and "order" in msg
    rc, msg = _rc(segs, 1024, 4, bf, order=5)
    assert rc == _lib.FA_E_INVAL
    # (N = 512, M = 1024): torch splits the key across blocks
    assert not C.config(512, 1024)[0]
    for elem in (_lib.FA_ELEM_F32, _lib.FA_ELEM_F16, bf):
        rc, msg = _rc(segs, 1024, 512, elem)
        assert rc == _lib.FA_E_RANGE and "outside the restated configurations" in msg
    rc, msg = _rc([[0, 1024], [512, 8]], 2048, 4, bf)
    assert rc == _lib.FA_E_INVAL and "overlapping" in msg and "16-bit" in msg
    rc, msg = _rc([[8, 1024]], 1024, 4, bf)
    assert rc == _lib.FA_E_INVAL and "outside bucket" in msg
    rc, msg = _rc(segs, -1, 4, bf)
    assert rc == _lib.FA_E_INVAL
    import ctypes
    a32, n32 = _lib.seg_array(np.asarray(segs, np.int64))
    assert L.fa_plan_build_order_host_elem(a32, n32, 1024, None, 0, 0, 4, 1, 0, bf, 0, None, None,
                                           0, None, None) == _lib.FA_E_INVAL
    arr = (_lib.FaTileDesc * 1)()
    nt = ctypes.c_int(0)
    lay = C.manifest_layout("bfloat16")
    b32, m32 = _lib.seg_array(lay.segs32)
    assert L.fa_plan_build_order_host_elem(b32, m32, lay.f32_numel, None, 0, 0, 4, 1, 0, bf, 0,
                                           arr, None, 1, None,
                                           ctypes.byref(nt)) == _lib.FA_E_RANGE
    assert nt.value > 1


def test_binding_refusals():
    """The create entry's argument checks run before any device call, so they
    hold without a GPU; Plan(elem=16-bit, order=TORCH_GPU) keeps raising."""
    segs = np.array([[0, 1024]], np.int64)
    for elem in (_lib.FA_ELEM_F16, _lib.FA_ELEM_BF16):
        with pytest.raises(_lib.FedaggError, match="16-bit"):
            _lib.Plan(segs, 1024, elem=elem, order=_lib.FA_ORDER_TORCH_GPU, n=4)
        with pytest.raises(_lib.FedaggError, match=r"outside 2\.\."):
            _lib.Plan.for_order(segs, 1024, n=1, elem=elem)
        with pytest.raises(_lib.FedaggError, match="outside the restated"):
            _lib.Plan.for_order(segs, 1024, n=512, elem=elem)
        with pytest.raises(_lib.FedaggError, match="unknown flag bits"):
            _lib.Plan.for_order(segs, 1024, n=4, elem=elem, flags=0x40)
        with pytest.raises(_lib.FedaggError, match="order 5"):
            _lib.Plan.for_order(segs, 1024, n=4, elem=elem, order=5)
    with pytest.raises(_lib.FedaggError, match="elem must be"):
        _lib.Plan.for_order(segs, 1024, n=4, elem=9)
    import ctypes
    a32, n32 = _lib.seg_array(segs)
    assert L.fa_plan_create_order_elem(a32, n32, 1024, None, 0, 0, 4, 1, 0, _lib.FA_ELEM_BF16,
                                       None) == _lib.FA_E_INVAL
    h = ctypes.c_void_p(1)
    assert L.fa_plan_create_order_elem(a32, n32, 1024, None, 0, 0, 1, 1, 0, _lib.FA_ELEM_BF16,
                                       ctypes.byref(h)) == _lib.FA_E_RANGE
    assert not h.value   # *out is cleared first


def test_engine_option_defaults_off_and_every_call_sets_it():
    import feddct_amd
    from feddct_amd import aggregate as A
    e = A.engine()
    try:
        assert e.native16_gpu_order is False and e.order_key == "torch_cpu"
        feddct_amd.set_summation_order("torch_gpu", native16=True)
        assert e.native16_gpu_order is True and e.order_key == "torch_gpu+native16"
        feddct_amd.set_summation_order("torch_gpu")
        assert e.native16_gpu_order is False and e.order_key == "torch_gpu"
        A.set_summation_order("torch_cpu", native16=True)
        assert e.order_key == "torch_cpu"
    finally:
        feddct_amd.set_summation_order("torch_cpu")
    assert e.native16_gpu_order is False


def test_stand_alone_check_program(tmp_path):
    """tests/host/tgpu16_host_check.cpp with plan_host.cpp under plain g++
    (no ROCm include path): the same entry over its own layouts, the fp32
    table against plan_tgpu's, the refusals.  Exit 0: every case held."""
    assert shutil.which("g++"), "g++ is needed to build the check program"
    exe = str(tmp_path / "tgpu16_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe,
                    os.path.join(ROOT, "tests", "host", "tgpu16_host_check.cpp"),
                    os.path.join(ROOT, "feddct_amd", "csrc", "plan_host.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases held" in r.stdout
