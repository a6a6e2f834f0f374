"""GPU: host-resident fp16 / bf16 rounds in 16-bit buckets.

A. 16-bit and mixed tile-subset plans (fa_plan_create_from_tiles_elem): the
   union of a layout's range plans, run into one poisoned result bucket,
   against the one full plan and the oracle, through the raw C ABI.
B. fa_narrow_f32 against torch's CPU ``.to(dtype)``, exhaustively at the
   rounding boundaries.
C. pipeline.HostPipeline on native 16-bit layouts, with and without an fp32
   master global: fresh data every round, into poisoned buckets.
D. The drop-in on host-resident model.half() / model.bfloat16() modules
   against the reference loop, the reference's own fixtures, the rounds that
   stay staged, and the refusals that must remain.

Expected values never come from the engine: every 16-bit value widened
exactly to fp32, oracle.torch_order's mean (or weighted sum) of those, then
torch's own CPU ``.to(dtype)``; or the reference loop on deep copies; or the
reference's recorded outputs (tests/golden/).  Comparison is bit for bit; a
NaN result only has to be a NaN."""
import copy
import ctypes
import os
import warnings
from functools import lru_cache

import numpy as np
import pytest
import torch

import feddct_amd
import h16ref as R
import hostlayouts as H
from conftest import ROOT
from feddct_amd import _lib, aggregate
from feddct_amd.aggregate import engine
from feddct_amd.layout import KIND_I64, BucketLayout
from feddct_amd.partition import i64_tiles, split_tiles
from helpers import StateModule
from oracle import torch_order as T
from oracle.torch_mirror import reference_loop
from test_gpu_h16_dropin import (assert_same_state, assert_staged, fill, gold_cases, manifest)
from test_gpu_h16_kernel import DATA, make_i64, make_inputs

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
ELEM = {"float16": _lib.FA_ELEM_F16, "bfloat16": _lib.FA_ELEM_BF16}
F32 = _lib.FA_ELEM_F32
PAD = _lib.FA_PLAN_GAPS_ARE_PADDING
GUARD = 128                      # elements on each side of every buffer
G16, G32, G64 = 0x5a5a, 0xdeadbeef, -0x0123456789abcdef


@pytest.fixture(scope="module", autouse=True)
def _device():
    torch.cuda.set_device(DEV)


@pytest.fixture(autouse=True)
def fresh_engine():
    aggregate._ENGINE = None
    yield
    aggregate._ENGINE = None


def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def to16(x32, dtype):
    """torch's CPU .to(dtype) of float32 values -> (uint16 bits, NaN mask)."""
    f = torch.from_numpy(np.ascontiguousarray(x32, np.float32).copy())
    return bits16(f.to(TDT[dtype])), np.isnan(np.asarray(x32, np.float32))


def assert_bits16(got, x32, dtype, what):
    """uint16 patterns == .to(dtype) of the fp32 values (a NaN: any NaN)."""
    wb, wn = to16(x32, dtype)
    got = np.ascontiguousarray(got, np.uint16).reshape(-1)
    wb, wn = wb.reshape(-1), wn.reshape(-1)
    assert np.array_equal(np.isnan(R.widen(got, dtype)), wn), (what, "NaN positions")
    bad = np.nonzero((got != wb) & ~wn)[0]
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], wb[bad[:5]])


def assert_bits32(got, x32, what):
    """uint32 patterns == the fp32 values' (a NaN: any NaN)."""
    got = np.ascontiguousarray(got, np.uint32).reshape(-1)
    want = np.ascontiguousarray(x32, np.float32).reshape(-1)
    wn = np.isnan(want)
    assert np.array_equal(np.isnan(got.view(np.float32)), wn), (what, "NaN positions")
    bad = np.nonzero((got != want.view(np.uint32)) & ~wn)[0]
    assert bad.size == 0, (what, bad.size, bad[:5])


# ========================================================= A. range plans ====
# Keys of 1 .. 16385 elements; the second 4097 and the 33 sit at odd offsets
# (every column of theirs is a scalar-cascade column, 17 scalar tiles between
# the vector tiles the cuts fall on); the bucket ends `residue` mod 8.
A_SEGS = [(0, 16385), (16385 + 123, 5), (16640, 2049), (18689 + 4, 4097), (22912, 4097),
          (27009 + 6, 33), (27136, 8), (27144, 1), (27264, 100), (27364 + 3, 1)]
A_END = 27368
A_SEGS64 = [(0, 1), (1, 5)]
A_N = [1, 3, 9, 128, 129]
A_PARTS = [2, 6, 64]
A_NONEMPTY = {2: 2, 6: 6, 64: 12}      # non-empty ranges of each cut (12 vector tiles on 256 B)
A_CASES = [(dt, n, w) for dt in sorted(TDT) for n in A_N for w in (False, True)]


def a_numel(residue):
    return A_END + (residue - A_END) % 8


class ABufs:
    """n 16-bit client buckets, a result bucket (16-bit, or fp32 for a mixed
    plan) and the int64 buckets on the device, each between guard bands."""

    def __init__(self, dtype, bits, x64, numel, wide):
        n = bits.shape[0]
        self.n, self.numel, self.dtype, self.wide = n, numel, dtype, wide
        self.row = (numel + 7) // 8 * 8 + 2 * GUARD
        host = np.full((n, self.row), G16, np.uint16)
        host[:, GUARD:GUARD + numel] = bits
        self.c16 = torch.from_numpy(host.view(np.int16)).to(DEV)
        self.n64 = x64.shape[1]
        h64 = np.full((n, self.n64 + 2 * GUARD), G64, np.int64)
        h64[:, GUARD:GUARD + self.n64] = x64
        self.c64 = torch.from_numpy(h64).to(DEV)
        self.a16 = _lib.ptr_array([self.c16.data_ptr() + 2 * (self.row * i + GUARD)
                                   for i in range(n)])
        self.a64 = _lib.ptr_array([self.c64.data_ptr() + 8 * ((self.n64 + 2 * GUARD) * i + GUARD)
                                   for i in range(n)])
        self.poison()

    def poison(self):
        if self.wide:
            o = np.full(self.numel + 2 * GUARD, G32, np.uint32).view(np.int32)
        else:
            o = np.full(self.row, G16, np.uint16).view(np.int16)
        self.out = torch.from_numpy(o).to(DEV)
        self.o64 = torch.full((self.n64 + 2 * GUARD,), G64, dtype=torch.int64, device=DEV)
        self.pout = self.out.data_ptr() + (4 if self.wide else 2) * GUARD
        self.p64 = self.o64.data_ptr() + 8 * GUARD

    def call(self, plan, flags=0, weights=None):
        w = None if weights is None else (ctypes.c_float * self.n)(*[float(v) for v in weights])
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        return _lib.lib.fa_reduce(plan.handle, self.a16, self.a64, self.n, w, self.pout, self.p64,
                                  flags, st)

    def snapshot(self):
        torch.cuda.synchronize()
        return [t.clone() for t in (self.c16, self.out, self.c64, self.o64)]

    def out_bits(self):
        torch.cuda.synchronize()
        o = self.out.cpu().numpy()
        o = o.view(np.uint32) if self.wide else o.view(np.uint16)
        return o[GUARD:GUARD + self.numel]

    def out64(self):
        return self.o64.cpu().numpy()[GUARD:GUARD + self.n64]

    def assert_guards(self, bits, x64, what):
        torch.cuda.synchronize()
        o = self.out.cpu().numpy()
        o, g = (o.view(np.uint32), G32) if self.wide else (o.view(np.uint16), G16)
        assert (o[:GUARD] == g).all() and (o[GUARD + self.numel:] == g).all(), (what, "out")
        c = self.c16.cpu().numpy().view(np.uint16)
        assert (c[:, :GUARD] == G16).all() and (c[:, GUARD + self.numel:] == G16).all(), what
        assert np.array_equal(c[:, GUARD:GUARD + self.numel], bits), (what, "a client was written")
        o64, c64 = self.o64.cpu().numpy(), self.c64.cpu().numpy()
        assert (o64[:GUARD] == G64).all() and (o64[GUARD + self.n64:] == G64).all(), what
        assert (c64[:, :GUARD] == G64).all() and (c64[:, GUARD + self.n64:] == G64).all(), what
        assert np.array_equal(c64[:, GUARD:GUARD + self.n64], x64), what


def a_oracle(bits, dtype, w):
    xf = R.widen(bits, dtype).astype(np.float32)      # exact
    out = np.zeros(bits.shape[1], np.float32)
    for o, m in A_SEGS:
        with np.errstate(all="ignore"):
            v = xf[:, o:o + m]
            out[o:o + m] = T.torch_mean0(v) if w is None else T.weighted_sum0(v, w)
    return out


@pytest.mark.parametrize("k,case", list(enumerate(A_CASES)))
def test_union_of_range_plans_is_the_full_plan(k, case):
    dtype, n, weighted = case
    residue = k % 8
    numel = a_numel(residue)
    assert numel % 8 == residue
    flags = PAD if k % 2 else 0          # gaps that are padding, gaps that are not
    data = "realistic" if weighted else DATA[k % len(DATA)]
    bits = bits16(make_inputs(dtype, n, data, numel, 77 + k))
    x64 = make_i64(n, 6, 77 + k).numpy()
    w = T.weights_from_sizes(np.random.default_rng(k).integers(10, 1000, n)) if weighted else None
    mean32 = a_oracle(bits, dtype, w)
    want64 = np.concatenate([T.mean_i64_trunc(x64[:, o:o + m]) for o, m in A_SEGS64])
    inside = np.zeros(numel, bool)
    for o, m in A_SEGS:
        inside[o:o + m] = True
    segs = np.asarray(A_SEGS, np.int64)
    info, tiles = _lib.build_tiles_host(segs, numel, A_SEGS64, 6, flags=flags, elem=ELEM[dtype])
    t32 = tiles[tiles[:, 2] < 4]
    assert (t32[:, 2] == 1).sum() >= 17 and (t32[:, 2] == 0).sum() >= 10
    for wide in (False, True):
        what = (dtype, n, weighted, residue, "mixed" if wide else "16-bit")
        out_elem = F32 if wide else ELEM[dtype]
        b = ABufs(dtype, bits, x64, numel, wide)

        def check(tag):
            got = b.out_bits()
            if wide:
                assert_bits32(got[inside], mean32[inside], (what, tag))
            else:
                assert_bits16(got[inside], mean32[inside], dtype, (what, tag))
            if not flags:
                assert (got[~inside] == (G32 if wide else G16)).all(), (what, tag, "wrote a gap")
            assert np.array_equal(b.out64(), want64), (what, tag)
            b.assert_guards(bits, x64, (what, tag))
            return got

        full = _lib.Plan(segs, numel, A_SEGS64, 6, flags=flags, elem=ELEM[dtype],
                         out_elem=F32 if wide else None)
        assert b.call(full, 0, w) == _lib.FA_OK, _lib.lib.fa_last_error()
        ref = check("full")
        for parts in A_PARTS:
            ranges = split_tiles(tiles, parts, numel, None, 128)
            assert sum(hi > lo for lo, hi, _ in ranges) == A_NONEMPTY[parts], "a multi-chunk cut"
            plans = [_lib.Plan.from_tiles(sel, numel, 6, info["tile_elems"], flags, ELEM[dtype],
                                          out_elem) for _, _, sel in ranges if len(sel)]
            plans.append(_lib.Plan.from_tiles(i64_tiles(tiles), numel, 6, info["tile_elems"],
                                              flags, ELEM[dtype], out_elem))
            for p in plans:
                assert _lib.lib.fa_plan_elem(p.handle) == ELEM[dtype]
                assert _lib.lib.fa_plan_out_elem(p.handle) == out_elem
            assert sum(p.info["ntiles"] for p in plans) == len(tiles)
            b.poison()
            for p in plans[::-1] if parts == 6 else plans:    # (any order of the chunks)
                assert b.call(p, 0, w) == _lib.FA_OK, _lib.lib.fa_last_error()
            got = check(("parts", parts))
            ok = inside & ~np.isnan(mean32)
            assert np.array_equal(got[ok], ref[ok]), (what, parts, "differs from the full plan")
            if parts == 2:
                # what a subset plan refuses changes no byte anywhere
                snap = b.snapshot()
                for fl in (_lib.FA_F_BCAST, _lib.FA_F_BCAST_ONLY, _lib.FA_F_SUM_ONLY,
                           _lib.FA_F_BCAST | _lib.FA_F_SUM_ONLY):
                    assert b.call(plans[0], fl, w) == _lib.FA_E_INVAL, fl
                ch = _lib.FaChain(0, n, None, None, numel)
                st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                assert _lib.lib.fa_reduce_chain(plans[0].handle, b.a16, n, None, ctypes.byref(ch),
                                                b.pout, 0, st) == _lib.FA_E_INVAL
                assert b"16-bit plan" in _lib.lib.fa_last_error()
                for s, t in zip(snap, b.snapshot()):
                    assert torch.equal(s, t), (what, "a refused call wrote")


def test_fp32_pair_makes_the_fp32_subset_plan():
    p = _lib.Plan.from_tiles([(0, 1024, 0), (1024, 4, 0)], 2048, 0, 1024, PAD, F32, F32)
    assert _lib.lib.fa_plan_elem(p.handle) == F32 == _lib.lib.fa_plan_out_elem(p.handle)
    assert p.info["ntiles"] == 2 and p.info["tile_elems"] == 1024
    p = _lib.Plan.from_tiles([(0, 2048, 0)], 4096, 0, 0, PAD, ELEM["bfloat16"])
    assert p.info["tile_elems"] == 2048 and p.launch_form(3) == (2048, 1, 1)


# ====================================================== B. fa_narrow_f32 ====
@lru_cache(maxsize=None)
def narrow_patterns(dtype):
    """fp32 inputs at every rounding boundary of the 16-bit format: for every
    finite magnitude h with a finite successor the midpoint of (h, h + 1) —
    an exact tie —, its two fp32 neighbours and h itself; the same around the
    overflow threshold (the midpoint of the largest finite value and the
    first value past it); half the smallest subnormal and its neighbours; both
    signs of all of them; then +-0, +-inf and NaNs."""
    lo, hi = R.adjacent_pairs(dtype)
    a, b = R.widen(lo, dtype), R.widen(hi, dtype)
    mid = ((a + b) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (a + b) / 2), "the midpoints are fp32 values"
    top = R.widen(np.array([R.FORMAT[dtype][3]], np.uint16), dtype)
    past = np.ldexp(1.0, 16 if dtype == "float16" else 128)
    thr = (top + past) / 2                                      # float64: 2^128 is no fp32
    thr32 = thr.astype(np.float32)
    assert np.isfinite(thr32).all() and np.array_equal(thr32.astype(np.float64), thr)
    tiny = (R.widen(np.array([1], np.uint16), dtype) / 2).astype(np.float32)
    pts = np.concatenate([mid, thr32, tiny])
    up = np.nextafter(pts, np.float32(np.inf))
    dn = np.nextafter(pts, np.float32(0))
    pos = np.concatenate([pts, up, dn, a.astype(np.float32), top.astype(np.float32)])
    spec = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000,
                     0x7f800001, 0xff800001, 0x7fffffff, 0x7fa00000, 0x00000001, 0x80000001,
                     0x007fffff, 0x7f7fffff, 0xff7fffff], np.uint32).view(np.float32)
    x = np.concatenate([pos, -pos, spec]).astype(np.float32)
    rng = np.random.default_rng(5)
    return x[rng.permutation(x.size)]


def run_narrow(src32, dtype, off, numel, pad=64):
    """fa_narrow_f32 on elements [off, off + numel) of a device copy of
    ``src32`` into the same elements of a poisoned 16-bit buffer with guard
    bands; returns the whole destination as uint16."""
    src = torch.from_numpy(np.ascontiguousarray(src32, np.float32)).to(DEV)
    total = off + numel + pad
    dst = torch.from_numpy(np.full(GUARD + total + GUARD, G16, np.uint16).view(np.int16)).to(DEV)
    assert off + numel <= src.numel()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib.fa_narrow_f32(src.data_ptr() + 4 * off, dst.data_ptr() + 2 * (GUARD + off),
                                ELEM[dtype], numel, st)
    assert rc == _lib.FA_OK, _lib.lib.fa_last_error()
    torch.cuda.synchronize()
    return dst.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("dtype", sorted(TDT))
def test_narrow_rounds_as_torch_rounds(dtype):
    x = narrow_patterns(dtype)
    assert x.size > 250000 and x.size % 8 != 0      # (a scalar tail after 120+ workgroups)
    got = run_narrow(x, dtype, 0, x.size)
    assert_bits16(got[GUARD:GUARD + x.size], x, dtype, dtype)
    assert (got[:GUARD] == G16).all() and (got[GUARD + x.size:] == G16).all()
    # the ties really are ties, and really go both ways
    wb, _ = to16(x, dtype)
    lo, hi = R.adjacent_pairs(dtype)
    mid = ((R.widen(lo, dtype) + R.widen(hi, dtype)) / 2).astype(np.float32)
    tb, _ = to16(mid, dtype)
    assert np.array_equal(tb, np.where(lo % 2 == 0, lo, hi)), "ties go to the even neighbour"
    sub_max = 0x03ff if dtype == "float16" else 0x007f
    assert ((wb & 0x7fff) <= sub_max).sum() > 1000, "subnormal results"
    inf = R.FORMAT[dtype][2]
    assert ((wb & 0x7fff) == inf).sum() >= 6, "overflow to +-inf"


@pytest.mark.parametrize("off", [0, 128])
@pytest.mark.parametrize("numel", [0, 1, 7, 8, 2047, 2048, 2049, 2048 * 3 + 5])
@pytest.mark.parametrize("dtype", sorted(TDT))
def test_narrow_lengths_and_offsets(dtype, numel, off):
    x = narrow_patterns(dtype)[1000:1000 + off + numel + 64]
    got = run_narrow(x, dtype, off, numel)
    lo = GUARD + off
    assert_bits16(got[lo:lo + numel], x[off:off + numel], dtype, (dtype, numel, off))
    assert (got[:lo] == G16).all() and (got[lo + numel:] == G16).all(), "wrote outside the range"


def test_narrow_refuses_on_device_pointers_too():
    src = torch.zeros(64, device=DEV)
    dst = torch.from_numpy(np.full(64, G16, np.uint16).view(np.int16)).to(DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = _lib.lib
    assert L.fa_narrow_f32(src.data_ptr(), dst.data_ptr(), F32, 8, st) == _lib.FA_E_INVAL
    assert L.fa_narrow_f32(src.data_ptr() + 4, dst.data_ptr(), ELEM["float16"], 8,
                           st) == _lib.FA_E_INVAL
    assert L.fa_narrow_f32(src.data_ptr(), dst.data_ptr() + 2, ELEM["bfloat16"], 8,
                           st) == _lib.FA_E_INVAL
    assert L.fa_narrow_f32(src.data_ptr(), None, ELEM["bfloat16"], 8, st) == _lib.FA_E_INVAL
    torch.cuda.synchronize()
    assert (dst.cpu().numpy().view(np.uint16) == G16).all()


# ======================================================= C. HostPipeline ====
S32 = 7.25                         # the fp32 global's sentinel; 16-bit buckets take G16
S64 = -3


def man16(name, dtype):
    man = H.SWEEP if name == "sweep" else H.LAYOUTS[name]
    return {"keys": [dict(e, dtype=dtype if e["dtype"] == "float32" else e["dtype"])
                     for e in man["keys"]]}


def layouts16(name, dtype, master):
    """(global's layout, clients' layout) of a hostlayouts manifest in
    ``dtype``."""
    ent = [(e["key"], e["shape"], e["dtype"]) for e in man16(name, dtype)["keys"]]
    cl = BucketLayout(ent, native16=True)
    if not master:
        return cl, cl
    gl = BucketLayout([(k, s, "float32" if d == dtype else d) for k, s, d in ent], master16=True)
    assert gl.f32_numel == cl.f32_numel and np.array_equal(gl.segs32, cl.segs32)
    return gl, cl


@lru_cache(maxsize=None)
def c_inputs(name, dtype, r, n):
    """Round r's clients: per client {key: uint16 bits / int64 values}."""
    out = []
    for i in range(n):
        rng = np.random.default_rng(100000 * r + 1000 * i + len(name) + (dtype == "float16"))
        st = {}
        for e in man16(name, dtype)["keys"]:
            m = int(np.prod(e["shape"])) if e["shape"] else 1
            if e["dtype"] == "int64":
                st[e["key"]] = rng.integers(0, 500, m)
            else:
                base = np.random.default_rng(len(e["key"]) + m).normal(0, 0.05, m)
                x = base * (1 + 0.01 * r + 0.02 * rng.normal(0, 1, m))
                st[e["key"]] = bits16(torch.from_numpy(x.astype(np.float32)).to(TDT[dtype]))
        out.append(st)
    return out


def c_weights(n):
    return T.weights_from_sizes(np.arange(1, n + 1) * 13 + 5)


@lru_cache(maxsize=None)
def c_want(name, dtype, r, n, weighted):
    """{key: the fp32 mean (floating keys) or the int64 result}."""
    ins = c_inputs(name, dtype, r, n)
    w = c_weights(n) if weighted else None
    out = {}
    for k in ins[0]:
        x = np.stack([s[k] for s in ins])
        if x.dtype == np.int64:
            out[k] = T.mean_i64_trunc(x)
        else:
            xf = R.widen(x, dtype).astype(np.float32)
            out[k] = T.torch_mean0(xf) if w is None else T.weighted_sum0(xf, w)
    return out


class Rows16:
    """Pinned host buckets: ``rows`` 16-bit ones (clients and broadcast
    targets), the global's (16-bit, or fp32 under a master), int64 ones."""

    def __init__(self, gl, cl, rows):
        self.gl, self.cl = gl, cl
        self.master = gl is not cl
        self.dtype = str(cl.float_dtype).replace("torch.", "")
        nf = max(cl.f32_numel, 64)
        self.b16 = torch.zeros(rows, nf, dtype=cl.float_dtype).pin_memory()
        self.g = torch.zeros(nf, dtype=gl.float_dtype).pin_memory()
        self.b64 = torch.zeros(rows, max(cl.i64_numel, 1), dtype=torch.int64).pin_memory()
        self.g64 = torch.zeros(max(cl.i64_numel, 1), dtype=torch.int64).pin_memory()

    def u16(self, row):
        return self.b16[row].view(torch.int16).numpy().view(np.uint16)

    def put(self, row, state):
        u = self.u16(row)
        for k, v in state.items():
            s = self.cl.by_key[k]
            dst = self.b64[row].numpy() if s.kind == KIND_I64 else u
            dst[s.offset:s.offset + s.numel] = v

    def poison(self, rows):
        for r in rows:
            self.u16(r)[:] = G16
            self.b64[r].fill_(S64)
        if self.g.dtype == torch.float32:
            self.g.fill_(S32)
        else:
            self.g.view(torch.int16).numpy().view(np.uint16)[:] = G16
        self.g64.fill_(S64)

    def check(self, want, targets, what):
        assert not self.master or self.g.dtype == torch.float32
        odd = 0
        for k, v in want.items():
            s = self.cl.by_key[k]
            sl = slice(s.offset, s.offset + s.numel)
            if s.kind == KIND_I64:
                assert np.array_equal(self.g64.numpy()[sl], v), (what, k, "global")
                for t in targets:
                    assert np.array_equal(self.b64[t].numpy()[sl], v), (what, k, t)
                continue
            if self.master:
                gb = self.g.numpy().view(np.uint32)[sl]
                assert_bits32(gb, v, (what, k, "the global: the unrounded fp32 mean"))
                odd += int((gb & 0xffff != 0).sum())
            else:
                gb = self.g.view(torch.int16).numpy().view(np.uint16)[sl]
                assert_bits16(gb, v, self.dtype, (what, k, "global"))
            for t in targets:
                assert_bits16(self.u16(t)[sl], v, self.dtype, (what, k, "target", t))
        if self.master and self.cl.f32_numel:
            assert odd > 0, "the fp32 global holds values no 16-bit element has"

    def untouched(self, rows):
        return all((self.u16(r) == G16).all() and (self.b64[r] == S64).all() for r in rows)


def c_round(pipe, rows, name, r, n, targets, weighted, fanout=None):
    ins = c_inputs(name, rows.dtype, r, n)
    for i, st in enumerate(ins):
        rows.put(i, st)
    targets = list(targets)
    rows.poison([t for t in targets if t >= n])
    pipe.run([rows.b16[i] for i in range(n)], [rows.b64[i] for i in range(n)], rows.g, rows.g64,
             [rows.b16[t] for t in targets], [rows.b64[t] for t in targets],
             weights=c_weights(n) if weighted else None, fanout=fanout)
    rows.check(c_want(name, rows.dtype, r, n, weighted), targets, (name, r, n, weighted))


def nonempty(ranges):
    for lo, hi, plan in ranges:
        assert (hi > lo) == (plan is not None), (lo, hi)
    return sum(hi > lo for lo, hi, _ in ranges)


@pytest.mark.parametrize("master", [False, True])
@pytest.mark.parametrize("n", [2, 9])
@pytest.mark.parametrize("nchunks,fanout", [(0, "host"), (0, "dma"), (6, "host"), (6, "dma"),
                                            (64, "host"), (64, "dma")])
@pytest.mark.parametrize("dtype", sorted(TDT))
def test_pipeline_three_fresh_rounds(dtype, nchunks, fanout, n, master):
    """mid: round 1 without a broadcast (ranges_nb), round 2 into two foreign
    buckets, round 3 into the clients' own input buckets (the reference's
    broadcast); weighted rounds alternate with unweighted ones."""
    from feddct_amd.pipeline import HostPipeline
    gl, cl = layouts16("mid", dtype, master)
    pipe = HostPipeline(cl, n, DEV, nchunks=nchunks, fanout=fanout, master=master)
    assert pipe.dev32[0].dtype == TDT[dtype] and pipe.dev32[0].numel() == cl.f32_numel
    assert pipe.out32.dtype == (torch.float32 if master else TDT[dtype])
    assert (pipe.out16 is not None) == master
    if master:
        assert pipe.out16.dtype == TDT[dtype] and pipe.out16.numel() == pipe.out32.numel()
    if nchunks == 0:
        assert nonempty(pipe.ranges) == 5 and nonempty(pipe.ranges_nb) == 2
    else:
        assert nonempty(pipe.ranges) >= 6 and pipe.ranges_nb is pipe.ranges
    for lo, hi, p in pipe.ranges:
        assert lo % 128 == 0
        if p is not None:
            assert p.elem == ELEM[dtype] and p.out_elem == (F32 if master else ELEM[dtype])
    assert pipe.plan64 is not None and pipe.plan64.elem == ELEM[dtype]
    rows = Rows16(gl, cl, n + 2)
    flip = n == 9
    c_round(pipe, rows, "mid", 1, n, (), flip)
    c_round(pipe, rows, "mid", 2, n, (n, n + 1), not flip)
    c_round(pipe, rows, "mid", 3, n, range(n), flip)


@pytest.mark.parametrize("name,dtype,master,fanout", [
    ("tiny", "bfloat16", True, "host"), ("onetile", "float16", True, "dma"),
    ("noi64", "bfloat16", False, "host"), ("noi64", "float16", True, "host"),
    ("nof32", "float16", False, "dma")])
def test_pipeline_edge_layouts(name, dtype, master, fanout):
    from feddct_amd.pipeline import HostPipeline
    n = 3
    gl, cl = layouts16(name, dtype, master)
    if name == "nof32":   # no floating key: nothing makes the layout 16-bit
        assert not cl.native16
        with pytest.raises(ValueError, match="native 16-bit"):
            HostPipeline(cl, n, DEV, master=True)
    pipe = HostPipeline(cl, n, DEV, fanout=fanout, master=master)
    assert len(pipe.ranges) == 5 and len(pipe.ranges_nb) == 2
    ne = nonempty(pipe.ranges)
    assert ne == 0 if name == "nof32" else ne >= 2 if name == "noi64" else ne == 1
    assert (pipe.plan64 is None) == (name == "noi64")
    rows = Rows16(gl, cl, n + 2)
    c_round(pipe, rows, name, 1, n, (n, n + 1), False)
    c_round(pipe, rows, name, 2, n, (), True)
    c_round(pipe, rows, name, 3, n, range(n), True, fanout="dma" if fanout == "host" else "host")


@pytest.mark.parametrize("master", [False, True])
def test_pipeline_checks_client_count_and_weights_length(master):
    from feddct_amd.pipeline import HostPipeline
    n = 3
    gl, cl = layouts16("mid", "bfloat16", master)
    pipe = HostPipeline(cl, n, DEV, master=master)
    rows = Rows16(gl, cl, n + 2)
    for i, st in enumerate(c_inputs("mid", "bfloat16", 1, n)):
        rows.put(i, st)
    rows.poison([n, n + 1])

    def run(k, weights):
        pipe.run([rows.b16[i] for i in range(k)], [rows.b64[i] for i in range(k)], rows.g,
                 rows.g64, [rows.b16[n], rows.b16[n + 1]], [rows.b64[n], rows.b64[n + 1]],
                 weights=weights)
    with pytest.raises(ValueError, match="built for 3 clients, got 2"):
        run(2, None)
    for bad in ([0.5, 0.25], [0.5, 0.25, 0.125, 0.125], []):
        with pytest.raises(ValueError, match=f"{len(bad)} weights for 3 clients"):
            run(n, bad)
    torch.cuda.synchronize()
    assert rows.untouched([n, n + 1])
    run(n, c_weights(n).reshape(n, 1))
    rows.check(c_want("mid", "bfloat16", 1, n, True), [n, n + 1], "after the refusals")


# ==================================================== D. host modules =======
def host_round(gman, cman, n, seed=0):
    """(reference global, reference clients, the engine's global, its
    clients): equal values, all on the host."""
    rg = fill(StateModule(gman), 999 + seed)
    rc = [fill(StateModule(cman), seed * 100 + i) for i in range(n)]
    return rg, rc, copy.deepcopy(rg), [copy.deepcopy(c) for c in rc]


def nudge_host(a_models, b_models, seed):
    """The same in-place update on both sides (a local training step)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for c, d in zip(a_models, b_models):
            for (k, v), w in zip(c.state_dict().items(), d.state_dict().values()):
                if v.dtype == torch.int64:
                    v.add_(3)
                    w.add_(3)
                else:
                    step = (torch.randn(v.shape, generator=g) * 0.01).to(v.dtype)
                    v.add_(step)
                    w.add_(step)


def assert_host_native(g, clients, tdt, mixed, dtypes):
    """The layout assertions the feature turns green: 16-bit pinned zero-copy
    arenas for host-resident modules, and no bound round."""
    ga = g._fa_arena
    if mixed:
        assert ga.layout.master16 and not ga.layout.native16 and ga.f32.dtype == torch.float32
    else:
        assert ga.layout.native16 and not ga.layout.master16 and ga.f32.dtype == tdt
    for m in clients:
        a = m._fa_arena
        assert a.layout.native16 and not a.layout.master16 and a.f32.dtype == tdt
        assert a.layout.f32_numel == ga.layout.f32_numel
    for m in [g] + list(clients):
        a = m._fa_arena
        assert a._packed == [] and a.valid()
        assert a.device.type == "cpu" and a.f32.is_pinned() and a.i64.is_pinned()
        for k, v in m.state_dict().items():
            assert v.device.type == "cpu" and v.dtype == dtypes[id(m)][k], k
    assert engine()._round is None, "host rounds stay unbound"


def dtypes_of(models):
    return {id(m): {k: v.dtype for k, v in m.state_dict().items()} for m in models}


def assert_round(rg, rc, g, cl, what):
    assert_same_state(rg, g, f"{what} global")
    for i in range(len(rc)):
        assert_same_state(rc[i], cl[i], f"{what} client {i}")


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("dtype", sorted(TDT))
def test_server_aggregate_on_host_modules(dtype, mixed):
    tdt, n = TDT[dtype], 9
    rg, rc, g, cl = host_round(manifest("float32" if mixed else dtype), manifest(dtype), n)
    dts = dtypes_of([g] + cl)
    for rnd in (1, 2):
        reference_loop(rg, rc)
        feddct_amd.server_aggregate(g, cl)
        assert_host_native(g, cl, tdt, mixed, dts)
        assert_round(rg, rc, g, cl, f"round {rnd}")
        if mixed:   # the global holds bits no 16-bit value has: the unrounded mean
            w = g.state_dict()["t5.w"]
            assert w.dtype == torch.float32 and not torch.equal(w, w.to(tdt).float())
        nudge_host(rc, cl, 7 + rnd)
    e = engine()
    kinds = [k for k in e._pipes if k[-1] == "<master>"]
    assert len(e._pipes) == 1 and len(kinds) == int(mixed)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("dtype", sorted(TDT))
def test_aggregate_weighted_on_host_modules(dtype, mixed):
    tdt, n = TDT[dtype], 9
    _, _, g, cl = host_round(manifest("float32" if mixed else dtype), manifest(dtype), n, seed=2)
    dts = dtypes_of([g] + cl)
    w = T.weights_from_sizes(np.arange(10, 10 + n))
    for rnd in (1, 2):
        ins = [{k: v.clone() for k, v in c.state_dict().items()} for c in cl]
        want = {}
        for k, v in g.state_dict().items():
            if v.dtype == torch.int64:
                want[k] = np.asarray(T.mean_i64_trunc(np.stack(
                    [c[k].numpy() for c in ins]))).reshape(v.shape)
            else:
                x = np.stack([c[k].float().numpy() for c in ins])
                want[k] = np.asarray(T.weighted_sum0(x, w), np.float32).reshape(v.shape)
        aggregate.aggregate_weighted(g, cl, weights=w, broadcast=rnd == 1)
        assert_host_native(g, cl, tdt, mixed, dts)
        for k, v in g.state_dict().items():
            if v.dtype == torch.int64:
                assert np.array_equal(v.numpy(), want[k]), k
            elif mixed:
                assert_bits32(v.view(torch.int32).numpy().view(np.uint32), want[k], k)
            else:
                assert_bits16(bits16(v), want[k], dtype, k)
        for i, c in enumerate(cl):
            for k, v in c.state_dict().items():
                if rnd == 2:     # broadcast=False: the clients keep their own values
                    assert torch.equal(v, ins[i][k]), (k, i)
                elif v.dtype == torch.int64:
                    assert np.array_equal(v.numpy(), want[k]), (k, i)
                else:
                    assert_bits16(bits16(v), want[k], dtype, (k, i))
        # the next round's inputs: every client steps away from the broadcast value
        g_ = torch.Generator().manual_seed(30 + rnd)
        with torch.no_grad():
            for c in cl:
                for v in c.state_dict().values():
                    if v.dtype == torch.int64:
                        v.add_(int(torch.randint(1, 9, (1,), generator=g_)))
                    else:
                        v.add_((torch.randn(v.shape, generator=g_) * 0.01).to(v.dtype))


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("dtype", sorted(TDT))
def test_two_model_call_on_host_modules(dtype, mixed):
    from test_gpu_h16_dropin import SHAPES
    tdt, n = TDT[dtype], 9
    gd = "float32" if mixed else dtype
    rgm, rcm, gm, clm = host_round(manifest(gd, SHAPES[:5], "m"), manifest(dtype, SHAPES[:5], "m"),
                                   n, seed=3)
    rgp, rcp, gp, clp = host_round(manifest(gd, SHAPES[4:], "p"), manifest(dtype, SHAPES[4:], "p"),
                                   n, seed=4)
    dts = dtypes_of([gm, gp] + clm + clp)
    for rnd in (1, 2):
        reference_loop(rgm, rcm)
        reference_loop(rgp, rcp)
        aggregate.server_aggregate_split(gm, gp, clm, clp)
        assert engine()._round is None
        pair = gm._fa_pairs[id(gp)]
        ga = pair._fa_arena
        assert (ga.layout.master16 if mixed else ga.layout.native16) and ga._packed == []
        assert ga.f32.dtype == (torch.float32 if mixed else tdt) and ga.f32.is_pinned()
        for a, b in zip(clm, clp):
            ca = a._fa_pairs[id(b)]._fa_arena
            assert ca.layout.native16 and ca._packed == [] and ca.f32.dtype == tdt
            assert ca.f32.is_pinned()
        for m in [gm, gp] + clm + clp:
            for k, v in m.state_dict().items():
                assert v.device.type == "cpu" and v.dtype == dts[id(m)][k], k
        assert_round(rgm, rcm, gm, clm, f"main {rnd}")
        assert_round(rgp, rcp, gp, clp, f"proxy {rnd}")
        nudge_host(rcm + rcp, clm + clp, 20 + rnd)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("dtype", sorted(TDT))
@pytest.mark.parametrize("n", [3, 17, 33])
def test_host_rounds_match_the_reference_fixtures(dtype, n, mixed):
    """The reference's own server_aggregate (tests/golden/): the clients' and
    a 16-bit global's bits from h16_goldens.npz, an fp32 global's from
    mixed16_goldens.npz; the modules stay on the host."""
    meta = gold_cases()
    gold16 = np.load(os.path.join(ROOT, "tests", "golden", "h16_goldens.npz"))
    gold = np.load(os.path.join(ROOT, "tests", "golden", "mixed16_goldens.npz"))
    tdt = TDT[dtype]

    def man(dt):
        return {"name": "g", "keys": [dict(e, dtype=dt if e["dtype"] == "h16" else e["dtype"])
                                      for e in meta["keys"]]}

    def load(m, tag):
        with torch.no_grad():
            for k, v in m.state_dict().items():
                t = torch.from_numpy(gold16[f"{dtype}/n{n}/{tag}/{k}"].copy())
                v.copy_(t if v.dtype == torch.int64 else t.view(tdt))
        return m
    cl = [load(StateModule(man(dtype)), f"in{i}") for i in range(n)]
    g = StateModule(man("float32" if mixed else dtype))
    dts = dtypes_of([g] + cl)
    feddct_amd.server_aggregate(g, cl)
    assert_host_native(g, cl, tdt, mixed, dts)
    for k, v in g.state_dict().items():
        if mixed:
            want = gold[f"{dtype}/n{n}/global/{k}"]
            got = v if v.dtype == torch.int64 else v.view(torch.int32)
        else:
            want = gold16[f"{dtype}/n{n}/out/{k}"]
            got = v if v.dtype == torch.int64 else v.view(torch.int16)
        assert np.array_equal(got.numpy(), want), k
    for c in cl:
        for k, v in c.state_dict().items():
            want = gold16[f"{dtype}/n{n}/out/{k}"]
            got = v if v.dtype == torch.int64 else v.view(torch.int16)
            assert np.array_equal(got.numpy(), want), k


# --------------------------------------------------------------- fallbacks ----
def staged_host_round(rg, rc, g, cl, what):
    reference_loop(rg, rc)
    feddct_amd.server_aggregate(g, cl)
    assert_staged([g] + cl)
    assert not g._fa_arena.layout.master16 and engine()._round is None
    assert_round(rg, rc, g, cl, what)


@pytest.mark.parametrize("gd", ["bfloat16", "float32"])
def test_fallback_clients_of_two_16_bit_dtypes(gd):
    rg, rc, g, cl = host_round(manifest(gd), manifest("bfloat16"), 4, seed=5)
    rc[2] = fill(StateModule(manifest("float16")), 77)
    cl[2] = copy.deepcopy(rc[2])
    staged_host_round(rg, rc, g, cl, "two dtypes")


@pytest.mark.parametrize("gd", ["bfloat16", "float32"])
def test_fallback_one_client_with_an_fp32_key(gd):
    man = manifest("bfloat16")
    rg, rc, g, cl = host_round(manifest(gd), man, 4, seed=6)
    odd = copy.deepcopy(man)
    odd["keys"][3]["dtype"] = "float32"
    rc[1] = fill(StateModule(odd), 78)
    cl[1] = copy.deepcopy(rc[1])
    staged_host_round(rg, rc, g, cl, "fp32-keyed client")


def test_fallback_the_inverse_mix():
    rg, rc, g, cl = host_round(manifest("float16"), manifest("float32"), 3, seed=8)
    staged_host_round(rg, rc, g, cl, "16-bit global, fp32 clients")


@pytest.mark.parametrize("gd", ["bfloat16", "float32"])
def test_client_with_an_extra_key_raises_where_the_reference_raises(gd):
    man = manifest("bfloat16")
    rg, rc, g, cl = host_round(manifest(gd), man, 4, seed=13)
    extra = copy.deepcopy(man)
    extra["keys"].append({"key": "more.w", "shape": [5], "dtype": "bfloat16"})
    rc[2] = fill(StateModule(extra), 79)
    cl[2] = copy.deepcopy(rc[2])
    before = [copy.deepcopy(c) for c in rc]
    with pytest.raises(RuntimeError, match="more.w"):
        reference_loop(rg, rc)
    with pytest.raises(RuntimeError, match="more.w"):
        feddct_amd.server_aggregate(g, cl)
    # the global loaded and the earlier clients updated through the unfused
    # broadcast (narrowing as torch's copy_ does); the raising client and the
    # later one as they were
    ga = g._fa_arena
    assert (ga.layout.master16 if gd == "float32" else ga.layout.native16) and ga._packed == []
    assert ga.f32.is_pinned()
    assert_same_state(rg, g, "global")
    for i in (0, 1):
        assert_same_state(rc[i], cl[i], f"client {i} updated")
        assert cl[i]._fa_arena.layout.native16 and cl[i]._fa_arena._packed == []
    for i in (2, 3):
        assert_same_state(before[i], cl[i], f"client {i} untouched")
    assert not torch.equal(rc[0].state_dict()["t5.w"], before[0].state_dict()["t5.w"])


@pytest.mark.parametrize("mixed", [False, True])
def test_a_set_that_moves_to_the_gpu_and_back_rebinds(mixed):
    tdt, n = torch.bfloat16, 3
    rg, rc, g, cl = host_round(manifest("float32" if mixed else "bfloat16"), manifest("bfloat16"),
                               n, seed=14)
    dts = dtypes_of([g] + cl)
    reference_loop(rg, rc)
    feddct_amd.server_aggregate(g, cl)
    assert_host_native(g, cl, tdt, mixed, dts)
    assert_round(rg, rc, g, cl, "host 1")
    nudge_host(rc, cl, 1)
    g, cl = g.to(DEV), [c.to(DEV) for c in cl]
    reference_loop(rg, rc)
    feddct_amd.server_aggregate(g, cl)
    rb = engine()._round
    assert rb is not None and rb.plan.elem == _lib.FA_ELEM_BF16
    assert rb.plan.out_elem == (F32 if mixed else _lib.FA_ELEM_BF16)
    assert all(m._fa_arena.device.type == "cuda" for m in [g] + cl)
    assert_round(rg, rc, g, cl, "device")
    g, cl = g.cpu(), [c.cpu() for c in cl]
    nudge_host(rc, cl, 2)
    dts = dtypes_of([g] + cl)
    reference_loop(rg, rc)
    feddct_amd.server_aggregate(g, cl)
    assert_host_native(g, cl, tdt, mixed, dts)
    assert_round(rg, rc, g, cl, "host 2")


def test_the_proximal_term_still_refuses_host_resident_16_bit_models():
    from feddct_amd.prox import ProximalTerm
    a, b = torch.nn.Linear(4, 3).half(), torch.nn.Linear(4, 3).half()
    with pytest.raises(NotImplementedError, match="supported pairs"):
        ProximalTerm(a, b)
    assert engine()._round_dtypes(a, [b]) == (None, None)


@pytest.mark.parametrize("mixed", [False, True])
def test_host_half_round_under_the_torch_gpu_order(mixed):
    tdt, n = torch.float16, 6
    rg, rc, g, cl = host_round(manifest("float32" if mixed else "float16"), manifest("float16"),
                               n, seed=15)
    dts = dtypes_of([g] + cl)
    reference_loop(rg, rc)
    feddct_amd.set_summation_order("torch_gpu")
    try:
        e = engine()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            feddct_amd.server_aggregate(g, cl)
        assert not [w for w in rec if issubclass(w.category, RuntimeWarning)]
        assert e.gpu_order_fallbacks == {}
        assert aggregate.summation_order() == "torch_gpu"
        assert_host_native(g, cl, tdt, mixed, dts)
    finally:
        feddct_amd.set_summation_order("torch_cpu")
    assert_round(rg, rc, g, cl, "torch_gpu order set")
