"""The 16-bit reduce kernels (csrc/fedagg_h16.hip) through the C ABI, against
the oracle: every value widened exactly to fp32, oracle.torch_order's
torch_mean0 (or weighted_sum0) on them, then torch's own CPU ``.to(dtype)``;
results compared as 16-bit integers, NaN positions as NaN."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from feddct_amd import _lib
from feddct_amd.layout import KIND_I64, BucketLayout
from oracle import torch_order as T

pytestmark = pytest.mark.gpu

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
NS = [1, 2, 3, 8, 9, 16, 17, 33, 129, 257]
SHAPES = [1, 7, 8, 31, 33, 100, 2047, 2049, 4097, 3 * 2048 + 40]
DATA = ["realistic", "cancel", "subnormal", "range", "naninf"]


@functools.lru_cache(maxsize=None)
def layout(dtype, shapes=tuple(SHAPES)):
    ent = [(f"t{j}", (m,), dtype) for j, m in enumerate(shapes)]
    ent.insert(2, ("nbt", (), "int64"))
    ent.append(("steps", (5,), "int64"))
    return BucketLayout(ent, native16=True)


@functools.lru_cache(maxsize=None)
def plan(dtype, shapes=tuple(SHAPES), tile=0):
    lay = layout(dtype, shapes)
    return _lib.Plan(lay.segs32, lay.f32_numel, lay.segs64, lay.i64_numel, tile_elems=tile,
                     elem=_lib.ELEM_OF_DTYPE[DTYPES[dtype]])


def from_bits(bits, tdt):
    return torch.from_numpy(np.asarray(bits, np.uint16).view(np.int16).copy()).view(tdt)


def bits_of(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def make_inputs(dtype, n, data, numel, seed):
    """[n, numel] client buckets of the 16-bit dtype (padding included: the
    kernels may reduce it, nothing reads its result)."""
    tdt = DTYPES[dtype]
    rng = np.random.default_rng(seed)
    sub_max = 0x03ff if dtype == "float16" else 0x007f   # largest subnormal's bits
    if data == "realistic":      # base + 1 % noise
        base = rng.normal(0, 0.05, numel)
        x = base[None, :] * (1 + 0.01 * rng.normal(0, 1, (n, numel)))
        return torch.from_numpy(x.astype(np.float32)).to(tdt)
    if data == "cancel":         # large values of both signs, small residue
        big = rng.normal(0, 1000.0, (n, numel))
        big[1::2] = -big[0::2][: big[1::2].shape[0]]
        x = big + rng.normal(0, 0.01, (n, numel))
        return torch.from_numpy(x.astype(np.float32)).to(tdt)
    if data == "subnormal":      # 16-bit subnormals, a few small normals among them
        bits = rng.integers(0, sub_max + 1, (n, numel)).astype(np.uint16)
        bits |= (rng.integers(0, 2, (n, numel)).astype(np.uint16) << 15)
        normal = rng.random((n, numel)) < 0.05
        bits[normal] += np.uint16(sub_max + 1)
        return from_bits(bits, tdt)
    if data == "range":
        # both ends of the format: means next to the largest finite value
        # (an unweighted mean of finite values cannot pass it: the overflow
        # endpoints are pinned in the weighted test) and means that land on a
        # 16-bit subnormal, ties included
        top = 0x7bff if dtype == "float16" else 0x7f7f
        bits = np.empty((n, numel), np.uint16)
        hi = top - rng.integers(0, 4, (n, numel))
        lo = (sub_max + 1) + rng.integers(0, 6, (n, numel))   # the smallest normals
        zero = np.zeros((n, numel), np.int64)
        pick = rng.integers(0, 4, numel)[None, :].repeat(n, 0)
        rowsel = rng.random((n, numel)) < 0.5
        bits[:] = np.where(pick == 0, hi, np.where(pick == 1, lo,
                           np.where(rowsel, lo, zero))).astype(np.uint16)
        sign = (pick == 3) & (rng.random((n, numel)) < 0.3)
        bits[sign] |= np.uint16(0x8000)
        return from_bits(bits, tdt)
    if data == "naninf":         # a NaN and an inf in one client
        x = rng.normal(0, 1.0, (n, numel)).astype(np.float32)
        c = int(rng.integers(0, n))
        x[c, 0::7] = np.nan
        x[c, 3::7] = np.inf
        x[c, 5::11] = -np.inf
        return torch.from_numpy(x).to(tdt)
    raise ValueError(data)


def make_i64(n, numel, seed):
    rng = np.random.default_rng(seed + 77)
    x = rng.integers(-1000, 1000, (n, numel))
    x[:, 0] = rng.integers(0, 1 << 40, n)   # beyond fp32's 24 bits
    return torch.from_numpy(x.astype(np.int64))


def expected(lay, tdt, x16, x64, weights=None):
    """Per key: the oracle on the widened inputs, then torch's CPU .to(dtype)."""
    xf = x16.float().numpy()
    out = {}
    for s in lay.slots:
        if s.kind == KIND_I64:
            out[s.key] = T.mean_i64_trunc(x64[:, s.offset:s.offset + s.numel].numpy()
                                          .reshape((-1,) + s.shape))
            continue
        v = xf[:, s.offset:s.offset + s.numel].reshape((-1,) + s.shape)
        with np.errstate(all="ignore"):
            r = T.torch_mean0(v) if weights is None else T.weighted_sum0(v, weights)
        out[s.key] = torch.from_numpy(np.ascontiguousarray(r, np.float32)).to(tdt)
    return out


def run(pl, x16, x64, weights=None, flags=0, out16=None, out64=None):
    n = x16.shape[0]
    dev = torch.device("cuda")
    c16, c64 = x16.to(dev), x64.to(dev)
    o16 = torch.full((x16.shape[1],), 1.0, dtype=x16.dtype, device=dev) if out16 is None else out16
    o64 = torch.full((max(x64.shape[1], 1),), -7, dtype=torch.int64, device=dev) \
        if out64 is None else out64
    a16 = _lib.ptr_array([c16[i].data_ptr() for i in range(n)])
    a64 = _lib.ptr_array([c64[i].data_ptr() for i in range(n)])
    w = None if weights is None else (ctypes.c_float * n)(*[float(v) for v in weights])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib.fa_reduce(pl.handle, a16, a64, n, w, o16.data_ptr(), o64.data_ptr(),
                                  flags, st), "fa_reduce")
    torch.cuda.synchronize()
    return o16, o64, c16, c64


def check(lay, tdt, o16, o64, want, what):
    for s in lay.slots:
        if s.kind == KIND_I64:
            got = o64[s.offset:s.offset + s.numel].cpu().numpy().reshape(s.shape)
            assert np.array_equal(got, want[s.key]), (what, s.key)
            continue
        got = o16[s.offset:s.offset + s.numel].cpu()
        exp = want[s.key].reshape(-1)
        gn, en = torch.isnan(got).numpy(), torch.isnan(exp).numpy()
        assert np.array_equal(gn, en), (what, s.key, "NaN positions")
        gb, eb = bits_of(got)[~gn], bits_of(exp)[~en]
        bad = np.nonzero(gb != eb)[0]
        assert bad.size == 0, (what, s.key, s.numel, bad[:5], gb[bad[:5]], eb[bad[:5]])


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_mean_matches_the_oracle(dtype, n, data):
    lay, tdt = layout(dtype), DTYPES[dtype]
    x16 = make_inputs(dtype, n, data, lay.f32_numel, 1000 * n + DATA.index(data))
    x64 = make_i64(n, lay.i64_numel, n)
    o16, o64, _, _ = run(plan(dtype), x16, x64)
    check(lay, tdt, o16, o64, expected(lay, tdt, x16, x64), (dtype, n, data))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_the_other_tile_width_gives_the_same_bits(dtype):
    lay, tdt = layout(dtype), DTYPES[dtype]
    x16 = make_inputs(dtype, 17, "realistic", lay.f32_numel, 5)
    x64 = make_i64(17, lay.i64_numel, 5)
    want = expected(lay, tdt, x16, x64)
    for tile in (2048, 4096):
        pl = plan(dtype, tile=tile)
        assert pl.info["tile_elems"] == tile and pl.launch_form(17)[0] == tile
        o16, o64, _, _ = run(pl, x16, x64)
        check(lay, tdt, o16, o64, want, (dtype, tile))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_third_cascade_level_at_4097_clients(dtype):
    """N = 4,097 on one small key: the second level's promotion into the
    third after 4,096 rows (body columns by the vector kernel's cascade, tail
    columns by the scalar ILP-4 order)."""
    shapes = (40,)
    lay, tdt = layout(dtype, shapes), DTYPES[dtype]
    n = 4097
    x16 = make_inputs(dtype, n, "cancel", lay.f32_numel, 9)
    x64 = make_i64(n, lay.i64_numel, 9)
    o16, o64, _, _ = run(plan(dtype, shapes), x16, x64)
    check(lay, tdt, o16, o64, expected(lay, tdt, x16, x64), (dtype, n))


@pytest.mark.parametrize("n", [3, 17, 129])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_weighted_matches_the_oracle(dtype, n):
    lay, tdt = layout(dtype), DTYPES[dtype]
    rng = np.random.default_rng(n)
    w = T.weights_from_sizes(rng.integers(10, 1000, n))
    for data in ("realistic", "cancel", "subnormal"):
        x16 = make_inputs(dtype, n, data, lay.f32_numel, 31 * n + DATA.index(data))
        x64 = make_i64(n, lay.i64_numel, n)
        o16, o64, _, _ = run(plan(dtype), x16, x64, weights=w)
        check(lay, tdt, o16, o64, expected(lay, tdt, x16, x64, w), (dtype, n, data, "weighted"))


def test_fp16_overflow_endpoints_round_as_torch_rounds_them():
    """65520.0 is the first fp32 value that rounds to fp16 inf, 65519.0 the
    last that rounds to the largest finite fp16 (0x7bff); both reached exactly
    as a weighted sum 2048 * w (+ 0 + 0), in a vector column and in scalar
    ones."""
    shapes = (64, 3, 1)
    lay = layout("float16", shapes)
    x = torch.zeros(3, lay.f32_numel, dtype=torch.float16)
    x[1] = 2048.0
    x64 = make_i64(3, lay.i64_numel, 1)
    for total, bits in ((65520.0, 0x7c00), (65519.0, 0x7bff), (-65520.0, 0xfc00),
                        (-65519.0, 0xfbff)):
        w = np.array([0.5, total / 2048.0, 0.25], np.float32)
        assert float(w[1]) * 2048.0 == total
        o16, o64, _, _ = run(plan("float16", shapes), x, x64, weights=w)
        for s in lay.slots:
            if s.kind != KIND_I64:
                assert (bits_of(o16[s.offset:s.offset + s.numel]) == bits).all(), (total, s.key)
        check(lay, torch.float16, o16, o64, expected(lay, torch.float16, x, x64, w), total)


@pytest.mark.parametrize("n", [1, 24, 25, 129])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_broadcast_copies_the_global_bytes_to_every_client(dtype, n):
    shapes = (1, 7, 100, 2049, 4097)
    lay, tdt = layout(dtype, shapes), DTYPES[dtype]
    pl = plan(dtype, shapes)
    x16 = make_inputs(dtype, n, "realistic", lay.f32_numel, n)
    x64 = make_i64(n, lay.i64_numel, n)
    want = expected(lay, tdt, x16, x64)
    o16, o64, c16, c64 = run(pl, x16, x64, flags=_lib.FA_F_BCAST)
    check(lay, tdt, o16, o64, want, (dtype, n, "bcast"))
    for i in range(n):
        assert np.array_equal(bits_of(c16[i]), bits_of(o16)), (n, i)
        assert torch.equal(c64[i], o64[:lay.i64_numel]), (n, i)
    # the broadcast alone: new global bytes into every client
    g16 = make_inputs(dtype, 1, "subnormal", lay.f32_numel, 99)[0].cuda()
    g64 = make_i64(1, lay.i64_numel, 99)[0].cuda()
    a16 = _lib.ptr_array([c16[i].data_ptr() for i in range(n)])
    a64 = _lib.ptr_array([c64[i].data_ptr() for i in range(n)])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib.fa_reduce(pl.handle, a16, a64, n, None, g16.data_ptr(), g64.data_ptr(),
                                  _lib.FA_F_BCAST_ONLY, st), "fa_reduce")
    torch.cuda.synchronize()
    for i in range(n):
        assert np.array_equal(bits_of(c16[i]), bits_of(g16)), (n, i)
        assert torch.equal(c64[i], g64), (n, i)


def test_refusals_on_a_16_bit_plan():
    lay = layout("bfloat16", (64,))
    pl = plan("bfloat16", (64,))
    assert _lib.lib.fa_plan_elem(pl.handle) == _lib.FA_ELEM_BF16
    assert pl.info["tile_elems"] in (2048, 4096)
    x = torch.zeros(2, lay.f32_numel, dtype=torch.bfloat16, device="cuda")
    x64 = torch.zeros(2, 8, dtype=torch.int64, device="cuda")
    a16 = _lib.ptr_array([x[i].data_ptr() for i in range(2)])
    a64 = _lib.ptr_array([x64[i].data_ptr() for i in range(2)])
    o, o64 = torch.zeros_like(x[0]), torch.zeros_like(x64[0])
    L = _lib.lib
    assert L.fa_reduce(pl.handle, a16, a64, 2, None, o.data_ptr(), o64.data_ptr(),
                       _lib.FA_F_SUM_ONLY, None) == _lib.FA_E_INVAL
    assert b"SUM_ONLY" in L.fa_last_error()
    ch = _lib.FaChain(0, 2, None, None, lay.f32_numel)
    assert L.fa_reduce_chain(pl.handle, a16, 2, None, ctypes.byref(ch), o.data_ptr(), 0,
                             None) == _lib.FA_E_INVAL
    assert b"16-bit" in L.fa_last_error()
    # a plan that does not own the whole bucket cannot broadcast it flat
    part = _lib.Plan(np.array([[0, 64]]), 1024, elem=_lib.FA_ELEM_BF16, flags=0)
    big = torch.zeros(2, 1024, dtype=torch.bfloat16, device="cuda")
    b16 = _lib.ptr_array([big[i].data_ptr() for i in range(2)])
    assert L.fa_reduce(part.handle, b16, None, 2, None, big[0].data_ptr(), None,
                       _lib.FA_F_BCAST, None) == _lib.FA_E_INVAL
    assert b"flat" in L.fa_last_error()
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0
