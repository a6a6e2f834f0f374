"""GPU: the reduce with its output aliasing a client bucket, and with a bucket
listed more than once.  include/fedagg.h promises of fa_reduce that out32 /
out64 "may alias a client bucket"; clients sampled with replacement, and a
global model that is itself one of the clients, reach the kernels as a
repeated pointer and as out == c[k].  Every result is compared bit for bit
with the oracle on host copies of the inputs taken before the call, every
bucket that must not change is compared bytewise, over a raw layout that holds
every column rule (empty, one-element and unaligned keys, cascade bodies, ILP-4
tails, a full and a partial vector tile, int64 keys), in both plan forms, at
client counts that take the inline pointers (1, 3, 17), the pointer table
(129) and the deep cascade (300), on the client-loop instances, through a
caller-owned table, the stateless entry points, the 16-bit plans and the
torch-GPU order."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from feddct_amd import synth
from feddct_amd.layout import KIND_H16, KIND_I64, Slot
from helpers import bits_equal
from longlaunch import long_launch_case
from oracle import torch_order as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)

# (numel, offset past the 64-float boundary): the 7-element key starts at an
# offset that is not a multiple of 4
KEYS32 = [(0, 0), (1, 0), (2, 0), (5, 0), (7, 1), (40, 0), (300, 0), (2048, 0), (2048 + 40, 0)]
KEYS64 = [1, 5, 33]
NMAX = 300
NS = [1, 3, 17, 129, 300]
FORMS = ["gaps", "table"]     # FA_PLAN_GAPS_ARE_PADDING; none of it + FA_PLAN_TUNE_NO_BALANCE
# (fa_reduce flags, weighted): FA_F_SUM_ONLY unweighted only
COMBOS = [("none", False), ("none", True), ("sum", False), ("bcast", False), ("bcast", True)]


@pytest.fixture(scope="module")
def lib():
    from feddct_amd import _lib
    torch.cuda.set_device(DEV)
    return _lib


def _round_up(x, a):
    return (x + a - 1) // a * a


@functools.lru_cache(maxsize=None)
def _layout():
    segs, off = [], 0
    for m, shift in KEYS32:
        off = _round_up(off, 64) + shift
        segs.append((off, m))
        off += m
    segs64, o64 = [], 0
    for m in KEYS64:
        segs64.append((o64, m))
        o64 += m
    return (np.array(segs, np.int64), _round_up(off, 64), np.array(segs64, np.int64),
            _round_up(o64, 2))


@functools.lru_cache(maxsize=None)
def _host():
    """NMAX adversarial client buckets on the host, read-only: client i's
    bucket is row i whatever the client count, gaps filled too (a key index of
    their own), so a written gap shows."""
    segs, numel, segs64, numel64 = _layout()
    x32 = np.stack([synth.gen_f32(90, numel, i, 0.0, 0.0, synth.MODE_ADVERSARIAL)
                    for i in range(NMAX)])
    x64 = np.stack([synth.gen_i64(91, numel64, i, synth.MODE_ADVERSARIAL) for i in range(NMAX)])
    for i in range(NMAX):
        for j, (o, m) in enumerate(segs):
            x32[i, o:o + m] = synth.gen_f32(j, int(m), i, 0.0, 0.0, synth.MODE_ADVERSARIAL)
        for j, (o, m) in enumerate(segs64):
            x64[i, o:o + m] = synth.gen_i64(20 + j, int(m), i, synth.MODE_ADVERSARIAL)
    x32.setflags(write=False)
    x64.setflags(write=False)
    return x32, x64


def _dev(a):
    """A fresh device copy of host rows (the host arrays are read-only)."""
    return torch.from_numpy(np.array(a)).to(DEV)


def _weights(n):
    return O.weights_from_sizes(np.arange(1, n + 1) * 7 + 3)


def _want(x32, x64, kind, w):
    """Per segment, the oracle on stacked host rows."""
    segs, _, segs64, _ = _layout()
    r32 = []
    for o, m in segs:
        cols = x32[:, o:o + m]
        if m == 0:
            r32.append(np.zeros(0, np.float32))
        elif w is not None:
            r32.append(O.weighted_sum0(cols, w))
        elif kind == "sum":
            r32.append(O.torch_sum0(cols))
        else:
            r32.append(O.torch_mean0(cols))
    return r32, [O.mean_i64_trunc(x64[:, o:o + m]) for o, m in segs64]


@functools.lru_cache(maxsize=None)
def _want_first(n, kind, weighted):
    x32, x64 = _host()
    return _want(x32[:n], x64[:n], kind, _weights(n) if weighted else None)


@functools.lru_cache(maxsize=None)
def _plan(form):
    from feddct_amd import _lib
    segs, numel, segs64, numel64 = _layout()
    flags = _lib.FA_PLAN_GAPS_ARE_PADDING if form == "gaps" else _lib.FA_PLAN_TUNE_NO_BALANCE
    return _lib.Plan(segs, numel, segs64, numel64, flags=flags)


def _flags(lib, kind):
    return {"none": 0, "sum": lib.FA_F_SUM_ONLY, "bcast": lib.FA_F_BCAST}[kind]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _wa(w):
    return None if w is None else (ctypes.c_float * len(w))(*[float(v) for v in w])


def _reduce(lib, plan, b32, b64, rows, w, out32, out64, flags):
    """fa_reduce over the buckets b32[r], b64[r] for r in rows (device
    [*, numel] tensors), into out32 / out64."""
    n = len(rows)
    lib.check(lib.lib.fa_reduce(plan.handle, lib.ptr_array([b32[r].data_ptr() for r in rows]),
                                lib.ptr_array([b64[r].data_ptr() for r in rows]), n, _wa(w),
                                out32.data_ptr(), out64.data_ptr(), flags, _stream()), "fa_reduce")
    torch.cuda.synchronize()


def _inside():
    segs, numel, segs64, numel64 = _layout()
    in32, in64 = np.zeros(numel, bool), np.zeros(numel64, bool)
    for o, m in segs:
        in32[o:o + m] = True
    for o, m in segs64:
        in64[o:o + m] = True
    return in32, in64


def _check_round(got32, got64, x32, x64, k, want, bcast, gaps, what):
    """got32 / got64: every bucket after the call (host, [rows, numel]);
    x32 / x64: the same buckets before it; bucket k took the result."""
    segs, _, segs64, _ = _layout()
    in32, in64 = _inside()
    w32, w64 = want
    for (o, m), v in zip(segs, w32):
        assert bits_equal(got32[k, o:o + m], v), (what, "f32 key", int(o), int(m))
    for (o, m), v in zip(segs64, w64):
        assert np.array_equal(got64[k, o:o + m], v), (what, "i64 key", int(o), int(m))
    u32, u0 = got32.view(np.uint32), x32.view(np.uint32)
    others = [r for r in range(got32.shape[0]) if r != k]
    if not gaps:      # nothing outside the segments is written, in any bucket
        assert np.array_equal(u32[:, ~in32], u0[:, ~in32]), (what, "fp32 gaps written")
        assert np.array_equal(got64[:, ~in64], x64[:, ~in64]), (what, "int64 gaps written")
    if bcast:
        for r in others:
            nan = np.isnan(got32[k])
            assert np.array_equal(np.isnan(got32[r]) & in32, nan & in32), (what, r)
            sel = in32 & ~nan
            assert np.array_equal(u32[r, sel], u32[k, sel]), (what, "broadcast f32", r)
            assert np.array_equal(got64[r, in64], got64[k, in64]), (what, "broadcast i64", r)
    else:             # every other client's bucket bytewise unchanged, gaps included
        assert np.array_equal(u32[others], u0[others]), (what, "another client's fp32 bucket")
        assert np.array_equal(got64[others], x64[others]), (what, "another client's int64 bucket")


def _aliased_cases():
    """Every N, every k in {0, N // 2, N - 1}, every (flags, weighting), the
    plan form alternating; and k = N - 1 once more in the other form: 90."""
    cases = []
    for i, n in enumerate(NS):
        for j, k in enumerate(sorted({0, n // 2, n - 1})):
            for c, (kind, weighted) in enumerate(COMBOS):
                form = FORMS[(i + j + c) % 2]
                cases.append((n, k, kind, weighted, form))
                if k == n - 1:
                    cases.append((n, k, kind, weighted, FORMS[(i + j + c + 1) % 2]))
    return cases


@pytest.mark.parametrize("n,k,kind,weighted,form", _aliased_cases())
def test_output_aliases_client_k(lib, n, k, kind, weighted, form):
    x32, x64 = _host()
    x32, x64 = x32[:n], x64[:n]
    b32, b64 = _dev(x32), _dev(x64)
    w = _weights(n) if weighted else None
    _reduce(lib, _plan(form), b32, b64, range(n), w, b32[k], b64[k], _flags(lib, kind))
    _check_round(b32.cpu().numpy(), b64.cpu().numpy(), x32, x64, k,
                 _want_first(n, kind, weighted), kind == "bcast", form == "gaps",
                 (n, k, kind, weighted, form))


@pytest.mark.parametrize("n", [3, 17, 256])
def test_client_loop_instances_in_place(lib, n):
    """The long launch of test_client_loop_instances_on_a_long_launch (pipe 1
    at 3 and 17 clients, 2 at 256): the call into a separate output first,
    then, on identical inputs, into client k's bucket — equal on every
    element — and the oracle on that test's windows."""
    layout, plan, x, windows = long_launch_case(lib, n, False, DEV)
    assert plan.launch_form(n, False)[2] == (2 if n >= 256 else 1)
    ptrs = lib.ptr_array([x[i].data_ptr() for i in range(n)])
    want = [O.torch_mean0(x[:, o:o + m].cpu().numpy()) for o, m in windows]
    for k in sorted({0, n - 1}):
        # the separate output starts as a copy of bucket k, so the elements
        # the plan does not own (the bucket's tail padding) compare too
        keep, sep = x[k].clone(), x[k].clone()
        lib.check(lib.lib.fa_reduce(plan.handle, ptrs, None, n, None, sep.data_ptr(), None, 0,
                                    _stream()), "fa_reduce")
        torch.cuda.synchronize()
        for (o, m), v in zip(windows, want):
            assert bits_equal(sep[o:o + m].cpu().numpy(), v), (n, k, o, m)
        lib.check(lib.lib.fa_reduce(plan.handle, ptrs, None, n, None, x[k].data_ptr(), None, 0,
                                    _stream()), "fa_reduce")
        torch.cuda.synchronize()
        assert torch.equal(x[k].view(torch.int32), sep.view(torch.int32)), (n, k)
        x[k].copy_(keep)      # identical inputs for the next k


@pytest.mark.parametrize("kind", ["none", "bcast"])
def test_caller_table_output_aliases_the_last_client(lib, kind):
    n, k = 129, 128
    x32, x64 = _host()
    x32, x64 = x32[:n], x64[:n]
    b32, b64 = _dev(x32), _dev(x64)
    table = torch.zeros(int(lib.lib.fa_table_bytes(n)), dtype=torch.uint8, device=DEV)
    assert table.data_ptr() % 8 == 0
    lib.check(lib.lib.fa_reduce_tab(_plan("gaps").handle,
                                    lib.ptr_array([b32[r].data_ptr() for r in range(n)]),
                                    lib.ptr_array([b64[r].data_ptr() for r in range(n)]), n, None,
                                    table.data_ptr(), b32[k].data_ptr(), b64[k].data_ptr(),
                                    _flags(lib, kind), _stream()), "fa_reduce_tab")
    torch.cuda.synchronize()
    _check_round(b32.cpu().numpy(), b64.cpu().numpy(), x32, x64, k,
                 _want_first(n, kind, False), kind == "bcast", True, ("tab", kind))


@pytest.mark.parametrize("entry", ["fa_mean_f32", "fa_weighted_f32", "fa_mean_i64_trunc"])
def test_stateless_entry_points_in_place(lib, entry):
    n, k = 9, 4
    segs, numel, segs64, numel64 = _layout()
    x32, x64 = _host()
    x32, x64 = x32[:n], x64[:n]
    in32, in64 = _inside()
    if entry == "fa_mean_i64_trunc":
        b = _dev(x64)
        arr, ns = lib.seg_array(segs64)
        lib.check(lib.lib.fa_mean_i64_trunc(lib.ptr_array([b[r].data_ptr() for r in range(n)]), n,
                                            numel64, b[k].data_ptr(), arr, ns, _stream()), entry)
        torch.cuda.synchronize()
        got = b.cpu().numpy()
        for (o, m), v in zip(segs64, _want_first(n, "none", False)[1]):
            assert np.array_equal(got[k, o:o + m], v), (entry, int(o))
        others = [r for r in range(n) if r != k]
        assert np.array_equal(got[others], x64[others])
        assert np.array_equal(got[k, ~in64], x64[k, ~in64])
        return
    b = _dev(x32)
    arr, ns = lib.seg_array(segs)
    ptrs = lib.ptr_array([b[r].data_ptr() for r in range(n)])
    weighted = entry == "fa_weighted_f32"
    if weighted:
        lib.check(lib.lib.fa_weighted_f32(ptrs, _wa(_weights(n)), n, numel, b[k].data_ptr(), arr,
                                          ns, _stream()), entry)
    else:
        lib.check(lib.lib.fa_mean_f32(ptrs, n, numel, b[k].data_ptr(), arr, ns, _stream()), entry)
    torch.cuda.synchronize()
    got = b.cpu().numpy()
    for (o, m), v in zip(segs, _want_first(n, "none", weighted)[0]):
        assert bits_equal(got[k, o:o + m], v), (entry, int(o), int(m))
    others = [r for r in range(n) if r != k]
    assert np.array_equal(got.view(np.uint32)[others], x32.view(np.uint32)[others])
    # a stateless plan does not write gaps
    assert np.array_equal(got.view(np.uint32)[k, ~in32], x32.view(np.uint32)[k, ~in32])


# ------------------------------------------------------------ 16-bit plans --
# (numel, offset past the 64-element boundary): a 6-element key (the 4-column
# body of a key of 4..7 elements takes the scalar cascade) and a 40-element key
# at an offset that is not a multiple of 8 (the scalar cascade too)
KEYS16 = [(1, 0), (6, 0), (40, 4), (300, 0), (2048 + 40, 0)]


class _Lay16:
    def __init__(self, tdt):
        self.slots, off = [], 0
        for j, (m, shift) in enumerate(KEYS16):
            off = _round_up(off, 64) + shift
            self.slots.append(Slot(f"t{j}", (m,), tdt, KIND_H16, off, m))
            off += m
        self.f32_numel = _round_up(off, 64)
        self.slots.append(Slot("nbt", (), torch.int64, KIND_I64, 0, 1))
        self.slots.append(Slot("steps", (5,), torch.int64, KIND_I64, 1, 5))
        self.i64_numel = 6
        self.segs32 = np.array([(s.offset, s.numel) for s in self.slots if s.kind == KIND_H16])
        self.segs64 = np.array([(s.offset, s.numel) for s in self.slots if s.kind == KIND_I64])


@pytest.mark.parametrize("kind", ["none", "bcast"])
@pytest.mark.parametrize("n", [3, 17, 129])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_16_bit_plans_in_place(lib, dtype, n, kind):
    import test_gpu_h16_kernel as H
    tdt = H.DTYPES[dtype]
    lay = _Lay16(tdt)
    assert any(s.offset % 8 for s in lay.slots if s.kind == KIND_H16)
    pl = lib.Plan(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel,
                  elem=lib.ELEM_OF_DTYPE[tdt])
    k = n - 1
    x16 = H.make_inputs(dtype, n, "cancel", lay.f32_numel, 50 + n)
    x64 = H.make_i64(n, lay.i64_numel, n)
    want = H.expected(lay, tdt, x16, x64)
    c16, c64 = x16.to(DEV), x64.to(DEV)
    H.run(pl, c16, c64, flags=_flags(lib, kind), out16=c16[k], out64=c64[k])
    H.check(lay, tdt, c16[k], c64[k], want, (dtype, n, kind))
    for r in range(n - 1):
        if kind == "bcast":   # the flat copy: the whole bucket's bytes
            assert np.array_equal(H.bits_of(c16[r]), H.bits_of(c16[k])), (dtype, n, r)
            assert torch.equal(c64[r], c64[k]), (dtype, n, r)
        else:
            assert np.array_equal(H.bits_of(c16[r]), H.bits_of(x16[r])), (dtype, n, r)
            assert torch.equal(c64[r].cpu(), x64[r]), (dtype, n, r)


# -------------------------------------------------------- torch-GPU order --
@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("n", [5, 32, 129])
def test_torch_gpu_order_in_place(lib, n, last):
    """The torch-GPU order's kernels (row splits, lanes meeting in a shuffle
    tree for the one-element fp32 keys and the int64 keys), output on client
    0 and on client N - 1, against torch's own stack(...).mean(0) on device
    copies made before the call."""
    segs, numel, segs64, numel64 = _layout()
    segs = segs[segs[:, 1] > 0]
    st = ctypes.c_int(0)
    assert lib.lib.fa_torch_gpu_config(n, 2048 + 40, ctypes.byref(st))
    assert st.value == (2 if n >= 32 else 1)     # N = 32 splits the large key's rows S = 2
    assert any(m == 1 for _, m in segs)
    plan = lib.Plan(segs, numel, segs64, numel64, order=lib.FA_ORDER_TORCH_GPU, n=n, flags=0)
    k = n - 1 if last else 0
    x32, x64 = _host()
    b32, b64 = _dev(x32[:n]), _dev(x64[:n])
    o32, o64 = b32.clone(), b64.clone()
    _reduce(lib, plan, b32, b64, range(n), None, b32[k], b64[k], 0)
    for o, m in segs:
        ref = torch.stack([o32[r, o:o + m].view(()) if m == 1 else o32[r, o:o + m]
                           for r in range(n)], 0).mean(0).reshape(-1)
        assert bits_equal(b32[k, o:o + m].cpu().numpy(), ref.cpu().numpy()), (n, k, int(o), int(m))
    for o, m in segs64:
        ref = torch.stack([(o64[r, o:o + m].view(()) if m == 1 else o64[r, o:o + m]).float()
                           for r in range(n)], 0).mean(0)
        want = torch.zeros(int(m), dtype=torch.int64, device=DEV)
        want.copy_(ref.reshape(-1))      # load_state_dict's copy_: fp32 -> int64 truncation
        assert torch.equal(b64[k, o:o + m], want), (n, k, int(o))
    others = [r for r in range(n) if r != k]
    assert torch.equal(b32[others].view(torch.int32), o32[others].view(torch.int32))
    assert torch.equal(b64[others], o64[others])
    in32, _ = _inside()
    gaps = torch.from_numpy(~in32).to(DEV)
    assert torch.equal(b32[k][gaps].view(torch.int32), o32[k][gaps].view(torch.int32))


# ------------------------------------------------------- repeated clients --
def _rows(which):
    if which == "aba":
        return [0, 1, 0]
    if which == "n17":
        return [[0, 1, 2, 1][i % 4] for i in range(17)]       # b0 b1 b2 b1 b0 ...
    return [(3 * i) % 7 for i in range(130)]                  # 7 distinct buckets


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", ["none", "bcast"])
@pytest.mark.parametrize("which", ["aba", "n17", "n130"])
def test_a_bucket_listed_more_than_once(lib, which, kind, weighted):
    rows = _rows(which)
    n, distinct = len(rows), max(rows) + 1
    form = FORMS[(n + weighted + (kind == "bcast")) % 2]
    x32, x64 = _host()
    x32, x64 = x32[:distinct], x64[:distinct]
    b32 = _dev(np.concatenate([x32, x32[:1]]))   # last row: the output
    b64 = _dev(np.concatenate([x64, x64[:1]]))
    w = _weights(n) if weighted else None
    _reduce(lib, _plan(form), b32, b64, rows, w, b32[distinct], b64[distinct], _flags(lib, kind))
    want = _want(x32[rows], x64[rows], kind, w)
    _check_round(b32.cpu().numpy(), b64.cpu().numpy(), np.concatenate([x32, x32[:1]]),
                 np.concatenate([x64, x64[:1]]), distinct, want, kind == "bcast", form == "gaps",
                 (which, kind, weighted, form))


@pytest.mark.parametrize("kind", ["none", "bcast"])
@pytest.mark.parametrize("form", FORMS)
def test_output_aliases_a_bucket_listed_twice(lib, form, kind):
    rows = [0, 1, 0]
    x32, x64 = _host()
    x32, x64 = x32[:2], x64[:2]
    b32, b64 = _dev(x32), _dev(x64)
    _reduce(lib, _plan(form), b32, b64, rows, None, b32[0], b64[0], _flags(lib, kind))
    _check_round(b32.cpu().numpy(), b64.cpu().numpy(), x32, x64, 0,
                 _want(x32[rows], x64[rows], kind, None), kind == "bcast", form == "gaps",
                 ("aliased twice", form, kind))
