"""fp16 / bf16 clients reduced into an fp32 master global in torch-ROCm's GPU
order: the parts that need no GPU — fa_plan_create_order_elem_out's export,
its two forwarding arms, its refusals (all before any device call), and the
engine option set_summation_order(..., native16=True, native16_master=True)."""
import ctypes

import numpy as np
import pytest

import feddct_amd
from feddct_amd import _lib
from feddct_amd import aggregate as A
from test_abi import header_functions

L = _lib.lib
F32, F16, BF16 = _lib.FA_ELEM_F32, _lib.FA_ELEM_F16, _lib.FA_ELEM_BF16
CPU, GPU = _lib.FA_ORDER_TORCH_CPU, _lib.FA_ORDER_TORCH_GPU


def segs_of(rows):
    return _lib.seg_array(np.array(rows, np.int64))


def test_new_symbol_is_declared_exported_and_bound():
    f = "fa_plan_create_order_elem_out"
    assert f in header_functions() and f in _lib.EXPORTS
    assert len(getattr(L, f).argtypes) == 12
    assert "out_elem" in _lib.Plan.for_order.__code__.co_varnames
    assert _lib.FA_PLAN_FLAGS_KNOWN == 0x1000000D   # the output type is no flag


# Bad arguments every arm refuses on the host: (segments, numel, n, flags).
BAD = [([[0, 10], [5, 10]], 20, 4, 0),      # overlapping segments
       ([[8, 1024]], 1024, 4, 0),           # a segment outside the bucket
       ([[0, 1024]], -1, 4, 0),             # a negative bucket size
       ([[0, 1024]], 1024, 4, 0x40),        # an unknown flag
       ([[0, 1024]], 1024, 1, 0),           # n outside 2.. (the torch-GPU order's rule)
       ([[0, 1024]], 1024, 512, 0)]         # outside the restatement (that order's too)


@pytest.mark.parametrize("order", [CPU, GPU, 5])
@pytest.mark.parametrize("elem", [F32, F16, BF16])
def test_equal_types_forward_to_the_order_entry(elem, order):
    for rows, numel, n, flags in BAD:
        segs, ns = segs_of(rows)
        h = ctypes.c_void_p(1)
        want_rc = L.fa_plan_create_order_elem(segs, ns, numel, None, 0, 0, n, order, flags, elem,
                                              ctypes.byref(h))
        want, want_h = L.fa_last_error(), h.value
        if want_rc not in (_lib.FA_E_INVAL, _lib.FA_E_RANGE):
            # the CPU order knows no n: the arguments are good, and the parent
            # went on to the device (a plan, or FA_E_HIP without one)
            assert order == CPU and n in (1, 512) and flags == 0
            if want_rc == _lib.FA_OK:
                L.fa_plan_destroy(h)
            continue
        h = ctypes.c_void_p(1)
        rc = L.fa_plan_create_order_elem_out(segs, ns, numel, None, 0, 0, n, order, flags, elem,
                                             elem, ctypes.byref(h))
        assert (rc, L.fa_last_error(), h.value) == (want_rc, want, want_h), (rows, n, flags)


@pytest.mark.parametrize("elem", [F16, BF16])
def test_cpu_order_forwards_to_the_mixed_entry(elem):
    for rows, numel, n, flags in BAD[:4]:
        segs, ns = segs_of(rows)
        h = ctypes.c_void_p(1)
        want_rc = L.fa_plan_create_elem_out(segs, ns, numel, None, 0, 0, 0, flags, elem, F32,
                                            ctypes.byref(h))
        want = L.fa_last_error()
        assert want_rc == _lib.FA_E_INVAL and not h.value
        h = ctypes.c_void_p(1)
        rc = L.fa_plan_create_order_elem_out(segs, ns, numel, None, 0, 0, n, CPU, flags, elem, F32,
                                             ctypes.byref(h))
        assert (rc, L.fa_last_error()) == (want_rc, want) and not h.value, (rows, flags)


@pytest.mark.parametrize("order", [CPU, GPU])
def test_every_other_pair_is_refused_with_out_cleared(order):
    segs, ns = segs_of([[0, 4096]])
    legal = {(F32, F32), (F16, F16), (BF16, BF16), (F16, F32), (BF16, F32)}
    for elem in (-1, F32, F16, BF16, 3, 16):
        for out_elem in (-1, F32, F16, BF16, 3, 16):
            if (elem, out_elem) in legal:
                continue
            h = ctypes.c_void_p(1)
            rc = L.fa_plan_create_order_elem_out(segs, ns, 4096, None, 0, 0, 4, order, 1, elem,
                                                 out_elem, ctypes.byref(h))
            assert rc == _lib.FA_E_INVAL and not h.value, (elem, out_elem)
            assert b"elem" in L.fa_last_error(), (elem, out_elem)


@pytest.mark.parametrize("elem", [F16, BF16])
def test_master_pair_refusals_need_no_device(elem):
    segs, ns = segs_of([[0, 4096]])

    def create(n=4, order=GPU, flags=1, numel=4096, out=None, s=segs, k=ns):
        h = ctypes.c_void_p(1)
        rc = L.fa_plan_create_order_elem_out(s, k, numel, None, 0, 0, n, order, flags, elem, F32,
                                             ctypes.byref(h) if out is None else out)
        return rc, L.fa_last_error(), h.value

    rc, msg, h = create(flags=0x40)
    assert rc == _lib.FA_E_INVAL and b"unknown flag bits" in msg and not h
    assert b"fa_plan_create_order_elem_out" in msg
    rc, msg, h = create(order=5)
    assert rc == _lib.FA_E_INVAL and b"order 5" in msg and not h
    for n in (-1, 0, 1, _lib.FA_MAX_CLIENTS + 1):
        rc, msg, h = create(n=n)
        assert rc == _lib.FA_E_RANGE and b"outside 2.." in msg and not h, n
    rc, msg, h = create(n=512, numel=1024, s=segs_of([[0, 1024]])[0])
    assert rc == _lib.FA_E_RANGE and b"outside the restated configurations" in msg and not h
    bad, nb = segs_of([[0, 10], [5, 10]])
    rc, msg, h = create(numel=20, s=bad, k=nb)
    assert rc == _lib.FA_E_INVAL and b"overlap" in msg and not h
    assert L.fa_plan_create_order_elem_out(segs, ns, 4096, None, 0, 0, 4, GPU, 1, elem, F32,
                                           None) == _lib.FA_E_INVAL
    assert b"NULL" in L.fa_last_error()


def test_binding_passes_the_output_type_through():
    segs = np.array([[0, 1024]], np.int64)
    for elem in (F16, BF16):
        with pytest.raises(_lib.FedaggError, match=r"fa_plan_create_order_elem_out.*outside 2\.\."):
            _lib.Plan.for_order(segs, 1024, n=1, elem=elem, out_elem=F32)
        with pytest.raises(_lib.FedaggError, match="outside the restated"):
            _lib.Plan.for_order(segs, 1024, n=512, elem=elem, out_elem=F32)
        with pytest.raises(_lib.FedaggError, match="unknown flag bits"):
            _lib.Plan.for_order(segs, 1024, n=4, elem=elem, out_elem=F32, flags=0x40)
    with pytest.raises(_lib.FedaggError, match="out_elem must equal elem"):
        _lib.Plan.for_order(segs, 1024, n=4, elem=F32, out_elem=BF16)
    with pytest.raises(_lib.FedaggError, match="out_elem must equal elem"):
        _lib.Plan.for_order(segs, 1024, n=4, elem=F16, out_elem=BF16)
    # the constructor's own rule stands: no torch-GPU order with an output type
    with pytest.raises(_lib.FedaggError, match="output element type"):
        _lib.Plan(segs, 1024, elem=F16, out_elem=F32, order=GPU, n=4)


def test_option_validates_and_gives_three_order_keys():
    e = A.engine()
    try:
        assert e.native16_master_gpu_order is False and e.order_key == "torch_cpu"
        with pytest.raises(ValueError, match="native16_master"):
            feddct_amd.set_summation_order("torch_gpu", native16_master=True)
        with pytest.raises(ValueError, match="native16_master"):
            A.set_summation_order("torch_cpu", native16=False, native16_master=True)
        with pytest.raises(ValueError, match="order must be"):
            feddct_amd.set_summation_order("torch", native16=True, native16_master=True)
        assert e.order_key == "torch_cpu" and e.native16_master_gpu_order is False
        keys = set()
        feddct_amd.set_summation_order("torch_gpu")
        keys.add(e.order_key)
        feddct_amd.set_summation_order("torch_gpu", native16=True)
        keys.add(e.order_key)
        assert e.order_key == "torch_gpu+native16"
        feddct_amd.set_summation_order("torch_gpu", native16=True, native16_master=True)
        keys.add(e.order_key)
        assert e.native16_gpu_order and e.native16_master_gpu_order
        assert keys == {"torch_gpu", "torch_gpu+native16", "torch_gpu+native16+master"}
        # every call sets it: option off after on restores the old key
        feddct_amd.set_summation_order("torch_gpu", native16=True)
        assert e.order_key == "torch_gpu+native16" and e.native16_master_gpu_order is False
        feddct_amd.set_summation_order("torch_gpu", strict=True, native16=True,
                                       native16_master=True)
        assert e.strict_gpu_order and e.order_key == "torch_gpu+native16+master"
        feddct_amd.set_summation_order("torch_gpu")
        assert e.order_key == "torch_gpu"
        # the CPU order is one key whatever the options say
        A.set_summation_order("torch_cpu", native16=True, native16_master=True)
        assert e.order_key == "torch_cpu"
    finally:
        feddct_amd.set_summation_order("torch_cpu")
    assert e.native16_gpu_order is False and e.native16_master_gpu_order is False


def test_plan_cache_key_tells_the_master_plan_from_the_pure_one():
    """Engine.plan(order="torch_gpu") keys its cache by master too: a cached
    refusal (None) of the pure plan must not answer for the master plan."""
    import torch
    from feddct_amd.layout import BucketLayout
    e = A.Engine()
    lay = BucketLayout([("w", (1024,), "bfloat16")], native16=True)
    dev = torch.device("cuda", 0)
    sentinel = object()
    e._gpu_plans[(lay.signature, 0, 4)] = None
    e._gpu_plans[(lay.signature, 0, 4, "<master>")] = sentinel
    assert e.plan(lay, dev, 4, "torch_gpu") is None
    assert e.plan(lay, dev, 4, "torch_gpu", master=True) is sentinel
