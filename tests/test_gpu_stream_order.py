"""Stream order of the C ABI (include/fedagg.h): every launch of every entry
point that takes a ``void *stream`` rides that stream.

Each case runs through tests/streamgate.py on a side stream, in arrangement A
(behind a running gate on the same stream, inputs poisoned before and after)
and B (a gate on the null stream, the side stream idle), and its results are
compared bit for bit with the reference its family's kernel test uses (the
oracle through test_gpu_reduce_tab / test_gpu_mixed16_kernel /
test_gpu_h16_kernel, torch's own GPU mean for the torch-GPU-order 16-bit
plans, float64 within the existing bounds for the prox kernels), guard bands
intact.  A launch that went to stream 0, or to an internal stream without a
join, computes from poison in A and has not run at the copy-out in B.

The pool path (fa_reduce with no table above FA_INLINE_CLIENTS, and what
reaches it) runs in B only: it uploads its table from a host vector that dies
at return, which is only sound where the runtime stages pageable uploads
before hipMemcpyAsync returns — a property of the runtime,
not something to establish by handing a kernel a freed table.

The torch-GPU-order fp32 cases: at n = 48 fa_torch_gpu_config puts every key
at a row split of 1 or 2, so two launches are all a plan of 48 clients has;
n = 64 (splits 1, 2, 4) and n = 129 through a table (1, 2, 4, 8) have three
and four, asserted from the host table and the plan info.

The CPU guard at the end parses both headers: an entry point with a stream
parameter, or a struct with a stream field, that is neither in the case table
nor in EXCLUDED with a reason fails the suite.
"""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import h16ref as R
import prox16ref as P
import streamgate as SG
import test_gpu_abi_kernels as AK
import test_gpu_h16_kernel as H
import test_gpu_mixed16_kernel as M16
import test_gpu_reduce_tab as RT
import tgpu16cases as C16
from feddct_amd import _lib
from oracle import torch_gpu_order as G
from oracle import torch_order as T

L = _lib.lib
OK = _lib.FA_OK
BCAST, BCAST_ONLY = _lib.FA_F_BCAST, _lib.FA_F_BCAST_ONLY
PAD = _lib.FA_PLAN_GAPS_ARE_PADDING
GUARD = RT.GUARD
N64 = RT.N64

CASES = {}      # name -> SimpleNamespace(entries, arrs, build)


def case(name, entries, arrs="AB"):
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = SimpleNamespace(entries=tuple(entries), arrs=arrs, build=fn)
        return fn
    return deco


def sp(st):
    return ctypes.c_void_p(st.cuda_stream)


def floats(w):
    return None if w is None else (ctypes.c_float * len(w))(*[float(v) for v in w])


# ===================================================== fp32, torch-CPU order ====
def _snap(res):
    return SimpleNamespace(o32=res.out[0].view(np.uint32), o64=res.out[1],
                           c32=res.out[2].view(np.uint32), c64=res.out[3])


def reduce32(n, weighted, flags, variant="pad", how="tab", inplace=False):
    """fa_reduce / fa_reduce_tab on test_gpu_reduce_tab's layout (vector tiles,
    ILP-4 tails, an M == 1 key, int64 keys) and its cached inputs and oracle.
    how: "tab" fa_reduce_tab (a caller's table above 128 clients), "pool"
    fa_reduce (above 128: the library's stream-ordered pool)."""
    lens = RT.LENS_DEEP if n > 4096 else RT.LENS
    c = RT.make(n, lens, variant)
    b = c.b
    what = ("reduce32", n, weighted, flags, variant, how, inplace)
    table = RT.Table(n) if how == "tab" else None
    a32, a64 = _lib.ptr_array(b.p32), _lib.ptr_array(b.p64)
    wa = floats(c.w) if weighted else None
    o32, o64 = (b.p32[0], b.p64[0]) if inplace else (b.out32, b.out64)
    if flags == BCAST_ONLY:
        rng = np.random.default_rng(n)
        g32 = rng.standard_normal(c.numel).astype(np.float32).view(np.uint32)
        g64 = rng.integers(-(1 << 50), 1 << 50, N64)
        b.load(g32, g64)
        inputs = [SG.In(b.o32), SG.In(b.o64)]
    else:
        inputs = [SG.In(b.c32), SG.In(b.c64)]

    def call(st):
        if how == "tab":
            rc = L.fa_reduce_tab(c.plan.handle, a32, a64, n, wa, table.ptr, o32, o64, flags, sp(st))
        else:
            rc = L.fa_reduce(c.plan.handle, a32, a64, n, wa, o32, o64, flags, sp(st))
        assert rc == OK, (what, L.fa_last_error())

    def check(res, arr):
        s = _snap(res)
        b.assert_guards(s, what)
        if table is not None:
            table.assert_guards(what)
        if flags == BCAST_ONLY:
            assert np.array_equal(RT.body32(b, s), g32) and np.array_equal(RT.body64(s), g64), \
                (what, "the broadcast wrote its source")
            RT.check_broadcast(c, s, g32, g64, what)
        elif inplace:
            RT.check_reduce(c, SimpleNamespace(o32=s.c32[0], o64=s.c64[0]), weighted, what)
            assert np.array_equal(s.c32[1:], b.h32[1:]) and np.array_equal(s.c64[1:], b.h64[1:]), \
                (what, "another client written")
            assert (s.o32 == RT.G32).all() and (s.o64 == RT.G64).all(), (what, "out bucket written")
        else:
            RT.check_reduce(c, s, weighted, what)
            if flags & BCAST:
                RT.check_broadcast(c, s, RT.body32(b, s), RT.body64(s), what)
            else:
                b.assert_clients_untouched(s, what)
        if arr == "A":
            SG.assert_poison2(res, inputs, what)

    return SimpleNamespace(call=call, inputs=inputs, outputs=[b.o32, b.o64, b.c32, b.c64],
                           check=check)


for _n in (2, 20, 128, 129, 321, 4097):
    for _w in (False, True):
        for _f in (0, BCAST):
            case(f"reduce32-n{_n}-{'w' if _w else 'mean'}-f{_f}", ["fa_reduce_tab"])(
                lambda n=_n, w=_w, f=_f: reduce32(n, w, f))
for _n in (2, 20):      # fa_reduce itself, inline
    case(f"reduce32-plain-n{_n}", ["fa_reduce"])(lambda n=_n: reduce32(n, n == 20, BCAST, how="pool"))
for _w in (False, True):
    for _f in (0, BCAST):
        case(f"reduce32-pool-n129-{'w' if _w else 'mean'}-f{_f}", ["fa_reduce"], arrs="B")(
            lambda w=_w, f=_f: reduce32(129, w, f, how="pool"))
for _n in (20, 129):
    case(f"reduce32-bcast-only-n{_n}", ["fa_reduce_tab"])(
        lambda n=_n: reduce32(n, False, BCAST_ONLY))
case("reduce32-gaps-n20-bcast", ["fa_reduce_tab"])(lambda: reduce32(20, True, BCAST, "gaps"))
case("reduce32-gaps-n129-bcast", ["fa_reduce_tab"])(lambda: reduce32(129, False, BCAST, "gaps"))
case("reduce32-inplace-n20", ["fa_reduce_tab"])(lambda: reduce32(20, False, 0, inplace=True))


# ===================================================== fp32, torch-GPU order ====
# Keys per client count and the launches their plan makes: one per row split
# its keys reach, except that the planner lets the S = 1 and S = 4 tiles ride
# in the S = 2 launch when that group holds the most tiles — so at n = 129
# four S = 4 keys stand against one S = 2 key.
_TG = (5, 33, 100, 130, 260, 2048 + 8, 4097)
TG_LENS = {48: _TG, 64: _TG, 129: (5, 33, 100, 130, 134, 138, 142, 260, 4097)}
TG_GROUPS = {48: 2, 64: 3, 129: 4}


def tg_groups(n, segs, numel, flags):
    _, _, lo = _lib.build_order_tiles_host(segs, numel, RT.SEGS64, N64, n=n, flags=flags)
    return sum(lo[g + 1] > lo[g] for g in range(5)), lo[5]


def test_torch_gpu_order_cases_have_their_launch_groups():
    """No GPU: the row-split groups of each torch-GPU-order case's plan, from
    the library's host table, so that a case cannot quietly become one launch;
    and n = 48 cannot have a third (every key's split is 1 or 2)."""
    for n, want in TG_GROUPS.items():
        segs, numel, flags = RT.layout(TG_LENS[n], "gaps")
        assert tg_groups(n, segs, numel, flags)[0] == want, n
    for m in list(range(2, 3000)) + [4096, 1 << 16, 1 << 20]:
        assert C16.config(48, m) in ((True, 1), (True, 2)), m
    assert TG_GROUPS[64] >= 3 and TG_GROUPS[129] >= 3


def reduce_tgpu(n, bcast):
    lens = TG_LENS[n]
    segs, numel, flags = RT.layout(lens, "gaps")
    for m in lens + tuple(m for _, m in RT.SEGS64):
        assert L.fa_torch_gpu_config(n, m, None) and G.supported(n, m), (n, m)
    cols, x64, _ = RT.inputs(n, lens, 2)
    b = RT.Bufs(RT.place(cols, segs, numel), x64, numel)
    plan = _lib.Plan(np.asarray(segs, np.int64), numel, RT.SEGS64, N64, flags=flags,
                     order=_lib.FA_ORDER_TORCH_GPU, n=n)
    groups, ntiles = tg_groups(n, segs, numel, flags)
    assert plan.info["ntiles"] == ntiles and groups == TG_GROUPS[n], (n, groups, plan.info)
    what = ("torch-gpu", n, bcast)
    table = RT.Table(n)
    a32, a64 = _lib.ptr_array(b.p32), _lib.ptr_array(b.p64)
    inputs = [SG.In(b.c32), SG.In(b.c64)]
    inside = RT.inside_mask(segs, numel)
    c = SimpleNamespace(b=b, flags=flags, numel=numel, inside=inside)

    def call(st):
        rc = L.fa_reduce_tab(plan.handle, a32, a64, n, None, table.ptr, b.out32, b.out64,
                             BCAST if bcast else 0, sp(st))
        assert rc == OK, (what, L.fa_last_error())

    def check(res, arr):
        s = _snap(res)
        b.assert_guards(s, what)
        table.assert_guards(what)
        out = RT.body32(b, s)
        want = np.concatenate([G.gpu_mean0(cols[:, a:a + m]) for a, m in RT.key_slices(lens)])
        RT.assert_bits(RT.gather(out, segs), want, what)
        assert (out[~inside] == RT.G32).all(), (what, "wrote a gap")
        for o, m in RT.SEGS64:
            assert np.array_equal(RT.body64(s)[o:o + m], G.gpu_mean_i64_trunc(x64[:, o:o + m])), what
        if bcast:
            RT.check_broadcast(c, s, out, RT.body64(s), what)
        else:
            b.assert_clients_untouched(s, what)
        if arr == "A":
            SG.assert_poison2(res, inputs, what)

    return SimpleNamespace(call=call, inputs=inputs, outputs=[b.o32, b.o64, b.c32, b.c64],
                           check=check)


for _n in sorted(TG_GROUPS):
    for _b in (False, True):
        case(f"tgpu32-n{_n}-{'bcast' if _b else 'reduce'}", ["fa_reduce_tab"])(
            lambda n=_n, b=_b: reduce_tgpu(n, b))


# ================================================================== 16-bit ====
def reduce16(dtype, form, n, weighted, flags=BCAST):
    """form: "pure" fa_plan_create_elem, "mixed" fa_plan_create_elem_out (the
    wide store + narrowing broadcast), "tgpu" fa_plan_create_order_elem,
    "tgpu-mixed" fa_plan_create_order_elem_out, "tiles" a subset through
    fa_plan_create_from_tiles_elem (no broadcast: a subset does not cover)."""
    segs, numel, pflags = M16.seg_list("aligned", 0)
    tdt, elem = M16.TDT[dtype], M16.ELEM[dtype]
    what = ("reduce16", dtype, form, n, weighted, flags)
    x16 = H.make_inputs(dtype, n, "realistic", numel, 1000 * n + weighted)
    bits = M16.bits_of16(x16)
    x64t = H.make_i64(n, N64, n)
    x64 = x64t.numpy()
    w = T.weights_from_sizes(np.random.default_rng(n).integers(10, 1000, n)) if weighted else None
    mixed = form in ("mixed", "tgpu-mixed")
    segs64 = M16.SEGS64
    covered = np.ones(numel, bool)
    if form == "mixed":
        plan = M16.mixed_plan(dtype, segs, numel, pflags, segs64, N64)
    elif form == "pure":
        plan = M16.pure_plan(dtype, segs, numel, pflags, segs64, N64)
    elif form == "tiles":
        _, tiles = _lib.build_tiles_host(segs, numel, elem=elem)
        sub = tiles[tiles[:, 2] < 4][::2]
        assert 2 <= len(sub) < len(tiles)
        plan = _lib.Plan.from_tiles(sub, numel, 0, elem=elem)
        covered[:] = False
        for s0, cnt, _ in sub:
            covered[s0:s0 + cnt] = True
        segs64 = []
    else:
        for m in [m for _, m in segs] + [m for _, m in segs64]:
            assert C16.config(n, m)[0], (n, m)
        plan = _lib.Plan.for_order(segs, numel, segs64, N64, n=n, elem=elem, flags=pflags,
                                   out_elem=_lib.FA_ELEM_F32 if mixed else None)
    b = M16.Bufs(dtype, bits, x64, numel)
    o16 = torch.from_numpy(np.full(b.row, M16.G16, np.uint16).view(np.int16)).cuda()
    out = b.p32 if mixed else o16.data_ptr() + 2 * M16.GUARD
    # the reference, once
    if form in ("tgpu", "tgpu-mixed"):       # torch's own GPU mean, as test_gpu_tgpu16_*_kernel
        dev16 = x16.cuda()
        want32 = np.concatenate([torch.stack([r.float() for r in dev16[:, o:o + m]], 0).mean(0)
                                 .cpu().numpy() for o, m in segs])
        want16 = np.concatenate([M16.bits_of16(
            torch.stack([r.float() for r in dev16[:, o:o + m]], 0).mean(0).to(tdt).cpu())
            for o, m in segs])
        d64 = x64t.cuda()
        want64 = np.zeros(N64, np.int64)
        for o, m in segs64:
            t = torch.zeros(m, dtype=torch.int64, device="cuda")
            t.copy_(torch.stack([r.float() for r in d64[:, o:o + m]], 0).mean(0))
            want64[o:o + m] = t.cpu().numpy()
        torch.cuda.synchronize()
    else:
        want32 = M16.oracle(bits, dtype, segs, w)
        exp = H.expected(RT.fake_layout(segs, M16.SEGS64), tdt, x16, x64t, w)
        want16 = np.concatenate([M16.bits_of16(exp[f"k{j}"]) for j in range(len(segs))])
        want64 = np.concatenate([T.mean_i64_trunc(x64[:, o:o + m]) for o, m in M16.SEGS64])
    assert not np.isnan(want32).any()
    wa = floats(w)
    inputs = [SG.In(b.c16, "f16bits" if dtype == "float16" else "bf16bits"), SG.In(b.c64)]
    a64 = b.a64 if segs64 else None
    p64 = b.p64 if segs64 else None
    G_ = M16.GUARD

    def call(st):
        rc = L.fa_reduce(plan.handle, b.a16, a64, n, wa, out, p64, flags, sp(st))
        assert rc == OK, (what, L.fa_last_error())

    def check(res, arr):
        o32, o64, h16, c16, c64 = res.out
        o32, h16, c16 = o32.view(np.uint32), h16.view(np.uint16), c16.view(np.uint16)
        assert (o32[:G_] == M16.G32).all() and (o32[G_ + numel:] == M16.G32).all(), (what, "out32")
        assert (h16[:G_] == M16.G16).all() and (h16[G_ + numel:] == M16.G16).all(), (what, "out16")
        assert (c16[:, :G_] == M16.G16).all() and (c16[:, G_ + numel:] == M16.G16).all(), what
        assert (o64[:G_] == M16.G64).all() and (o64[G_ + N64:] == M16.G64).all(), (what, "out64")
        assert (c64[:, :G_] == M16.G64).all() and (c64[:, G_ + N64:] == M16.G64).all(), what
        cb = c16[:, G_:G_ + numel]
        if segs64:
            assert np.array_equal(o64[G_:G_ + N64], want64), (what, "int64")
        else:
            assert (o64 == M16.G64).all(), (what, "int64 bucket written")
        if mixed:
            o = o32[G_:G_ + numel]
            M16.assert_f32_bits(M16.gather(o, segs), want32, what)
            assert (h16 == M16.G16).all(), (what, "the 16-bit bucket written")
            if flags & BCAST:
                M16.assert_narrowed(cb, o, dtype, what)
        else:
            o = h16[G_:G_ + numel]
            got, keep = M16.gather(o, segs), M16.gather(covered, segs)
            assert np.array_equal(got[keep], want16[keep]), what
            assert (o[~covered] == M16.G16).all(), (what, "outside the plan's tiles")
            assert (o32 == M16.G32).all(), (what, "the fp32 bucket written")
            if flags & BCAST:
                assert (cb == o[None, :]).all(), (what, "flat broadcast of the 16-bit bucket")
        if flags & BCAST:
            assert (c64[:, G_:G_ + N64] == want64[None, :]).all(), what
        else:
            assert np.array_equal(cb, bits), (what, "the reduce wrote a client")
        if arr == "A":
            SG.assert_poison2(res, inputs, what)

    return SimpleNamespace(call=call, inputs=inputs, outputs=[b.o32, b.o64, o16, b.c16, b.c64],
                           check=check)


for _d in sorted(M16.TDT):
    for _n in (5, 33):
        for _form in ("pure", "mixed"):
            for _w in (False, True):
                case(f"reduce16-{_form}-{_d}-n{_n}-{'w' if _w else 'mean'}", ["fa_reduce"])(
                    lambda d=_d, n=_n, f=_form, w=_w: reduce16(d, f, n, w))
        for _form in ("tgpu", "tgpu-mixed"):
            case(f"reduce16-{_form}-{_d}-n{_n}", ["fa_reduce"])(
                lambda d=_d, n=_n, f=_form: reduce16(d, f, n, False))
    case(f"reduce16-tiles-{_d}-n5", ["fa_reduce"])(lambda d=_d: reduce16(d, "tiles", 5, True, 0))


@case("narrow-f32-float16", ["fa_narrow_f32"])
def _narrow16():
    return narrow("float16")


@case("narrow-f32-bfloat16", ["fa_narrow_f32"])
def _narrowbf():
    return narrow("bfloat16")


def narrow(dtype):
    numel = 4099
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(numel) * 10.0 ** rng.integers(-3, 3, numel)).astype(np.float32)
    src = AK.Guarded(numel, x)
    row = (numel + 7) // 8 * 8 + 2 * GUARD
    dst = torch.from_numpy(np.full(row, M16.G16, np.uint16).view(np.int16)).cuda()
    want, _ = M16.to16(x.view(np.uint32), dtype)
    inputs = [SG.In(src.t)]

    def call(st):
        assert L.fa_narrow_f32(src.ptr(), dst.data_ptr() + 2 * GUARD, M16.ELEM[dtype], numel,
                               sp(st)) == OK, L.fa_last_error()

    def check(res, arr):
        h = res.out[0].view(np.uint16)
        assert np.array_equal(h[GUARD:GUARD + numel], want), dtype
        assert (h[:GUARD] == M16.G16).all() and (h[GUARD + numel:] == M16.G16).all(), "guards"
        if arr == "A":
            SG.assert_poison2(res, inputs, ("narrow", dtype))

    return SimpleNamespace(call=call, inputs=inputs, outputs=[dst], check=check)


# =================================================================== chain ====
def chain(weighted):
    """Three segments (n_total = 20 cut 7 + 7 + 6) queued back to back, the
    state planes carried on the device; the plan holds the layout's vector
    tiles (test_gpu_chain.py's _plans)."""
    n, cuts = 20, [0, 7, 14, 20]
    c = RT.make(n, RT.LENS, "pad")
    b = c.b
    _, tiles = _lib.build_tiles_host(np.asarray(c.segs, np.int64), c.numel, (), 0)
    vec = tiles[tiles[:, 2] == 0]
    assert len(vec) >= 3
    plan = _lib.Plan(None, c.numel, None, 0, 0, tiles=vec)
    covered = np.zeros(c.numel, bool)
    for s0, cnt, _ in vec:
        covered[s0:s0 + cnt] = True
    plane = (c.numel + 3) // 4 * 4
    state = torch.full((4 * plane,), float("nan"), device="cuda")
    w = c.w if weighted else None
    arrs = [_lib.ptr_array(b.p32[a:z]) for a, z in zip(cuts, cuts[1:])]
    was = [floats(w[a:z]) if weighted else None for a, z in zip(cuts, cuts[1:])]
    chs = [_lib.FaChain(a, n, state.data_ptr() if a else None,
                        state.data_ptr() if z < n else None, plane) for a, z in zip(cuts, cuts[1:])]
    inputs = [SG.In(b.c32)]
    what = ("chain", weighted)

    def call(st):
        for k, (a, z) in enumerate(zip(cuts, cuts[1:])):
            rc = L.fa_reduce_chain(plan.handle, arrs[k], z - a, was[k], ctypes.byref(chs[k]),
                                   b.out32 if z == n else None, 0, sp(st))
            assert rc == OK, (what, k, L.fa_last_error())

    def check(res, arr):
        o32, c32 = res.out[0].view(np.uint32), res.out[1].view(np.uint32)
        assert (o32[:GUARD] == RT.G32).all() and (o32[GUARD + c.numel:] == RT.G32).all(), what
        out = o32[GUARD:GUARD + c.numel]
        full = np.full(c.numel, RT.G32, np.uint32)
        ref = RT.reference(n, c.lens, "wsum" if weighted else "mean", c.seed)
        col = 0
        for o, m in c.segs:
            full[o:o + m] = ref[col:col + m].view(np.uint32)
            col += m
        seg = covered & c.inside
        assert seg.sum() > 4096
        assert np.array_equal(out[seg], full[seg]), what
        assert (out[~covered] == RT.G32).all(), (what, "outside the vector tiles")
        assert np.array_equal(c32, b.h32), (what, "a client written")
        if arr == "A":
            SG.assert_poison2(res, inputs, what)

    return SimpleNamespace(call=call, inputs=inputs, outputs=[b.o32, b.c32], check=check)


case("chain-mean", ["fa_reduce_chain"])(lambda: chain(False))
case("chain-weighted", ["fa_reduce_chain"])(lambda: chain(True))


# =============================================================== stateless ====
def stateless(fn):
    """fa_mean_f32 / fa_weighted_f32 / fa_mean_i64_trunc: called once first,
    so the internal plan cache is warm (plan creation uploads synchronously)."""
    n = 20
    if fn == "fa_mean_i64_trunc":
        segs, numel = [(0, 1), (1, 5), (8, 33)], 41
        rng = np.random.default_rng(9)
        x = rng.integers(-(1 << 40), 1 << 40, (n, numel)).astype(np.int64)
        want = np.concatenate([T.mean_i64_trunc(x[:, o:o + m]) for o, m in segs])
        src = AK.Guarded(numel, x, rows=n, i64=True)
        dst = AK.Guarded(numel, i64=True)
        sent = AK.G64
    else:
        c = RT.make(n, RT.LENS, "gaps")
        segs, numel = c.segs, c.numel
        cols, _, w = RT.inputs(n, c.lens, c.seed)
        want = RT.reference(n, c.lens, "mean" if fn == "fa_mean_f32" else "wsum", c.seed)
        src = AK.Guarded(numel, RT.place(cols, segs, numel), rows=n)
        dst = AK.Guarded(numel)
        sent = AK.G32
    sa, ns = _lib.seg_array(np.asarray(segs, np.int64))
    ptrs = _lib.ptr_array([src.ptr(r) for r in range(n)])
    wa = floats(w) if fn == "fa_weighted_f32" else None
    inputs = [SG.In(src.t)]
    inside = RT.inside_mask(segs, numel)

    def call(st):
        if fn == "fa_weighted_f32":
            rc = L.fa_weighted_f32(ptrs, wa, n, numel, dst.ptr(), sa, ns, sp(st))
        else:
            rc = getattr(L, fn)(ptrs, n, numel, dst.ptr(), sa, ns, sp(st))
        assert rc == OK, (fn, L.fa_last_error())

    call(torch.cuda.current_stream())              # warm the plan cache
    torch.cuda.synchronize()
    dst.t.copy_(torch.from_numpy(np.full((1, dst.row), sent, dst.dt)
                                 .view(np.int64 if dst.i64 else np.int32)))
    torch.cuda.synchronize()

    def check(res, arr):
        h = res.out[0].view(dst.dt)
        body = h[0, GUARD:GUARD + numel]
        assert (h[:, :GUARD] == sent).all() and (h[:, GUARD + numel:] == sent).all(), (fn, "guards")
        got = RT.gather(body, segs)
        if dst.i64:
            assert np.array_equal(got, want), fn
        else:
            RT.assert_bits(got, want, fn)
        assert (body[~inside] == sent).all(), (fn, "wrote a gap")
        if arr == "A":
            SG.assert_poison2(res, inputs, fn)

    return SimpleNamespace(call=call, inputs=inputs, outputs=[dst.t], check=check)


for _fn in ("fa_mean_f32", "fa_weighted_f32", "fa_mean_i64_trunc"):
    case(f"stateless-{_fn}", [_fn])(lambda fn=_fn: stateless(fn))


# =========================================================== small kernels ====
def div(inplace, trunc):
    numel, d = 4096 * 3 + 257, np.float32(7)
    x = AK.div_inputs(numel, 5)
    if trunc:
        with np.errstate(all="ignore"):
            q = x / d
        ok = np.isfinite(q) & (q >= np.float32(-2.0 ** 63)) & (q < np.float32(2.0 ** 63))
        x = np.where(ok, x, np.float32(-7.9))
    with np.errstate(all="ignore"):
        want = x / d
    src = AK.Guarded(numel, x)
    dst = src if inplace else AK.Guarded(numel, i64=trunc)
    inputs = [SG.In(src.t)]
    what = ("div", inplace, trunc)

    def call(st):
        fn = L.fa_div_trunc_i64 if trunc else L.fa_div_f32
        assert fn(src.ptr(), float(d), dst.ptr(), numel, sp(st)) == OK, L.fa_last_error()

    def check(res, arr):
        h = res.out[0].view(dst.dt)
        body = h[0, GUARD:GUARD + numel]
        assert (h[:, :GUARD] == dst.g).all() and (h[:, GUARD + numel:] == dst.g).all(), what
        if trunc:
            assert np.array_equal(body, np.trunc(want).astype(np.int64)), what
        else:
            AK.assert_f32(body, want, what)
        if arr == "A":
            SG.assert_poison2(res, inputs, what)

    return SimpleNamespace(call=call, inputs=inputs, outputs=[dst.t], check=check)


case("div-f32", ["fa_div_f32"])(lambda: div(False, False))
case("div-f32-inplace", ["fa_div_f32"])(lambda: div(True, False))
case("div-trunc-i64", ["fa_div_trunc_i64"])(lambda: div(False, True))


def broadcast(n):
    numel = 4099
    bits = AK.finite_bits(numel, n)
    src = AK.Guarded(numel, bits)
    dst = AK.Guarded(numel, rows=n)
    arr_ = _lib.ptr_array([dst.ptr(r) for r in range(n)])
    inputs = [SG.In(src.t)]

    def call(st):
        assert L.fa_broadcast_f32(src.ptr(), arr_, n, numel, sp(st)) == OK, L.fa_last_error()

    def check(res, arr):
        h = res.out[0].view(np.uint32)
        assert (h[:, GUARD:GUARD + numel] == bits[None, :]).all(), ("broadcast", n)
        assert (h[:, :GUARD] == AK.G32).all() and (h[:, GUARD + numel:] == AK.G32).all(), "guards"
        if arr == "A":
            SG.assert_poison2(res, inputs, ("broadcast", n))

    return SimpleNamespace(call=call, inputs=inputs, outputs=[dst.t], check=check)


case("broadcast-n3", ["fa_broadcast_f32"])(lambda: broadcast(3))
case("broadcast-n24", ["fa_broadcast_f32"])(lambda: broadcast(24))


@case("copy-f32", ["fa_copy_f32"])
def _copy():
    numel = 4099
    bits = AK.finite_bits(numel, 1)
    src, dst = AK.Guarded(numel, bits), AK.Guarded(numel)
    inputs = [SG.In(src.t)]

    def call(st):
        assert L.fa_copy_f32(src.ptr(), dst.ptr(), numel, sp(st)) == OK, L.fa_last_error()

    def check(res, arr):
        h = res.out[0].view(np.uint32)[0]
        assert np.array_equal(h[GUARD:GUARD + numel], bits)
        assert (h[:GUARD] == AK.G32).all() and (h[GUARD + numel:] == AK.G32).all(), "guards"
        if arr == "A":
            SG.assert_poison2(res, inputs, "copy")

    return SimpleNamespace(call=call, inputs=inputs, outputs=[dst.t], check=check)


def synth_fill(i64):
    """The output is the only operand: the sentinel logic alone applies."""
    from feddct_amd import synth
    numel = 4099
    dst = AK.Guarded(numel, i64=i64)
    if i64:
        want = synth.gen_i64(3, numel, 2, synth.MODE_ADVERSARIAL)
    else:
        want = synth.gen_f32(3, numel, 2, 0.0, 0.0, synth.MODE_ADVERSARIAL)

    def call(st):
        if i64:
            rc = L.fa_synth_fill_i64(dst.ptr(), numel, 3, 2, synth.MODE_ADVERSARIAL, sp(st))
        else:
            rc = L.fa_synth_fill_f32(dst.ptr(), numel, 3, 2, 0.0, 0.0, synth.MODE_ADVERSARIAL, sp(st))
        assert rc == OK, L.fa_last_error()

    def check(res, arr):
        h = res.out[0].view(dst.dt)[0]
        assert (h[:GUARD] == dst.g).all() and (h[GUARD + numel:] == dst.g).all(), "guards"
        body = h[GUARD:GUARD + numel]
        if i64:
            assert np.array_equal(body, want)
        else:
            assert np.array_equal(body, AK.f32_bits(want))

    return SimpleNamespace(call=call, inputs=[], outputs=[dst.t], check=check)


case("synth-fill-f32", ["fa_synth_fill_f32"])(lambda: synth_fill(False))
case("synth-fill-i64", ["fa_synth_fill_i64"])(lambda: synth_fill(True))


# ==================================================================== prox ====
PROX_LENGTHS = [1, 5, 1023, 0, 4097, 8193, 7]       # ragged, a one-element segment


def prox32(what, flags=0):
    import test_gpu_prox_edges as PE
    segs, numel = PE._place(PROX_LENGTHS)
    pc = PE._Case(segs, numel)
    g = torch.Generator(device="cuda").manual_seed(31)
    b = torch.randn(numel, device="cuda", generator=g)
    a = b + 0.01 * torch.randn(numel, device="cuda", generator=g)
    ia, ib = SG.In(a), SG.In(b)
    if what == "norms":
        norms = torch.full((pc.nseg + 2,), -7.0, device="cuda")
        total = torch.full((3,), -7.0, device="cuda")

        def call(st):
            _lib.check(L.fa_prox_norms(pc.plan.handle, a.data_ptr(), b.data_ptr(),
                                       norms[1:].data_ptr(), total[1:].data_ptr(), sp(st)))

        def check(res, arr):
            nr, tt = torch.from_numpy(res.out[0]), torch.from_numpy(res.out[1])
            assert nr[0] == -7 and nr[-1] == -7 and tt[0] == -7 and tt[2] == -7, "guards"
            PE._check_norms(pc, ia.real, ib.real, (nr[1:1 + pc.nseg], tt[1]), "stream-order")
            if arr == "A":
                SG.assert_poison2(res, [ia, ib], "prox norms")

        return SimpleNamespace(call=call, inputs=[ia, ib], outputs=[norms, total], check=check)
    (norms, _), = PE._norms(pc, a, b)
    gout = PE._gout(0.7)
    ga = torch.randn(numel, device="cuda", generator=g)
    gb = torch.randn(numel, device="cuda", generator=g)
    inputs = [ia, ib, SG.In(norms), SG.In(gout.reshape(1)), SG.In(ga), SG.In(gb)]
    d = PE._ref_d(pc, a, b, norms, gout, 1.0)

    def call(st):
        args = (pc.plan.handle, a.data_ptr(), b.data_ptr(), norms.data_ptr(), gout.data_ptr(), 1.0,
                ga.data_ptr(), gb.data_ptr())
        if what == "grad":
            _lib.check(L.fa_prox_grad(*args, sp(st)))
        else:
            _lib.check(L.fa_prox_grad_ex(*args, flags, sp(st)))

    def check(res, arr):
        PE._check_grad(pc, d, torch.from_numpy(res.out[0]), torch.from_numpy(res.out[1]),
                       inputs[4].real, inputs[5].real, flags, True, f"stream-order {what} {flags}")
        if arr == "A":
            SG.assert_poison2(res, inputs, ("prox", what, flags))

    return SimpleNamespace(call=call, inputs=inputs, outputs=[ga, gb], check=check)


case("prox-norms", ["fa_prox_norms"])(lambda: prox32("norms"))
case("prox-grad", ["fa_prox_grad"])(lambda: prox32("grad"))
case("prox-grad-ex-acc-a", ["fa_prox_grad_ex"])(lambda: prox32("ex", _lib.FA_PROX_ACCUMULATE_A))
case("prox-grad-ex-acc-b", ["fa_prox_grad_ex"])(lambda: prox32("ex", _lib.FA_PROX_ACCUMULATE_B))
case("prox-grad-ex-acc", ["fa_prox_grad_ex"])(lambda: prox32("ex", _lib.FA_PROX_ACCUMULATE))


def prox16(dtype, mixed, what):
    """fa_prox_norms_elem / fa_prox_grad_elem with a 16-bit anchor (pure) and
    an fp32 one (mixed), on prox16ref's ragged list (one-element and empty
    segments), checked as test_gpu_prox16_kernel checks them."""
    import test_gpu_prox16_kernel as PK
    from test_gpu_prox_edges import GRAD_BOUND, norm_bound, total_bound
    dt = PK.TORCH_DT[dtype]
    segs, numel = P.place(P.LENGTHS)
    assert 1 in [int(m) for _, m in segs]
    ab, bb = P.inputs(numel, 0, dtype, same=[tuple(segs[P.ZERO_SEG])])
    pc = PK._Case(segs, numel)
    a = PK._t(ab, dtype)
    g = torch.Generator(device="cuda").manual_seed(41)
    if mixed:
        b = PK._t(bb, dtype).float() + 0.001 * torch.randn(numel, device="cuda", generator=g)
    else:
        b = PK._t(bb, dtype)
    ia, ib = SG.In(a), SG.In(b)
    e_a, e_b = PK._elem(dtype), PK._elem("float32" if mixed else dtype)
    tdt = torch.float32 if mixed else dt
    name = ("prox16", dtype, mixed, what)
    if what == "norms":
        norms = torch.full((pc.nseg + 2,), -7.0, device="cuda")
        total = torch.full((3,), -7.0, device="cuda", dtype=tdt)

        def call(st):
            _lib.check(L.fa_prox_norms_elem(pc.plan.handle, a.data_ptr(), e_a, b.data_ptr(), e_b,
                                            norms[1:].data_ptr(), total[1:].data_ptr(), sp(st)))

        def check(res, arr):
            nr = res.out[0]
            assert nr[0] == -7 and nr[-1] == -7, "norms guard"
            nr = nr[1:1 + pc.nseg]
            if mixed:
                tt = res.out[1]
                assert tt[0] == -7 and tt[2] == -7, "total guard"
                dd = ia.real.cpu().double() - ib.real.cpu().double()
                want = torch.stack([(dd[o:o + m] ** 2).sum().sqrt() for o, m in pc.segs])
                lim = torch.tensor([norm_bound(c) for c in pc.chunks], dtype=torch.float64) * want
                assert bool(((torch.from_numpy(nr).double() - want).abs() <= lim).all()), name
                assert abs(float(tt[1]) - float(want.sum())) <= \
                    total_bound(pc.chunks) * float(want.sum()), name
            else:
                tb = res.out[1].view(np.uint16)
                guard = int(PK._bits(torch.tensor([-7.0]).to(dt))[0])
                assert tb[0] == guard and tb[2] == guard, "total guard"
                _, _, iv = P.exact_share(pc.segs, ab, bb, dtype)
                nb = P.rn16(nr, dtype)
                assert np.array_equal(P.f32(nb, dtype), nr), "norms[] are not 16-bit values"
                for k, (lo, hi) in enumerate(iv):
                    assert lo <= int(nb[k]) <= hi, (name, k)
                assert int(tb[1]) == P.running_total(nb, dtype), name
            if arr == "A":
                SG.assert_poison2(res, [ia, ib], name)

        return SimpleNamespace(call=call, inputs=[ia, ib], outputs=[norms, total], check=check)
    norms, _ = PK._norms(pc, a, b, dtype, mixed)
    gout = torch.tensor([0.7], device="cuda").to(tdt)
    ga = torch.randn(numel, device="cuda", generator=g).to(dt)
    gb = torch.randn(numel, device="cuda", generator=g).to(tdt)
    inputs = [ia, ib, SG.In(norms), SG.In(gout), SG.In(ga), SG.In(gb)]
    inside = pc.inside().numpy()

    def call(st):
        _lib.check(L.fa_prox_grad_elem(pc.plan.handle, a.data_ptr(), e_a, b.data_ptr(), e_b,
                                       norms.data_ptr(), gout.data_ptr(), 1.0, ga.data_ptr(),
                                       gb.data_ptr(), 0, sp(st)))

    def check(res, arr):
        pa, pb = SG._np(inputs[4].real.cpu()), SG._np(inputs[5].real.cpu())
        got_a, got_b = res.out[0].view(np.uint16), res.out[1]
        assert np.array_equal(got_a[~inside], pa.view(np.uint16)[~inside]), (name, "gap of grad_a")
        if mixed:
            assert np.array_equal(got_b.view(np.uint32)[~inside], pb.view(np.uint32)[~inside]), name
            diff = ia.real.cpu().double() - ib.real.cpu().double()
            d = torch.zeros(numel, dtype=torch.float64)
            nk = inputs[2].real.cpu().double()
            for k, (o, m) in enumerate(pc.segs):
                if m and float(nk[k]) != 0.0:
                    d[o:o + m] = float(inputs[3].real.cpu().double()) * diff[o:o + m] / nk[k]
            err = (torch.from_numpy(got_b).double() + d).abs()[inside]
            assert bool((err <= GRAD_BOUND * d.abs()[inside]).all()), name
            assert np.array_equal(got_a[inside], P.rn16(-got_b[inside], dtype)), name
        else:
            got_b = got_b.view(np.uint16)
            assert np.array_equal(got_b[~inside], pb.view(np.uint16)[~inside]), (name, "gap")
            want = PK._torch_grad16(pc, ia.real, ib.real, inputs[2].real, inputs[3].real[0], 1.0, dt)
            assert np.array_equal(got_a[inside], PK._bits(want)[inside]), name
            assert np.array_equal(got_b[inside], P.neg16(got_a[inside])), name
        if arr == "A":
            SG.assert_poison2(res, inputs, name)

    return SimpleNamespace(call=call, inputs=inputs, outputs=[ga, gb], check=check)


for _d in ("float16", "bfloat16"):
    for _m in (False, True):
        case(f"prox16-norms-{_d}-{'f32anchor' if _m else 'pure'}", ["fa_prox_norms_elem"])(
            lambda d=_d, m=_m: prox16(d, m, "norms"))
        case(f"prox16-grad-{_d}-{'f32anchor' if _m else 'pure'}", ["fa_prox_grad_elem"])(
            lambda d=_d, m=_m: prox16(d, m, "grad"))


# ================================================================== probes ====
@case("write-probe", ["fa_write_probe_f32"], arrs="B")
def _write_probe():
    n, numel, seed = 25, 4099, 0x9e3779b9
    dst = AK.Guarded(numel, rows=n)
    arr_ = _lib.ptr_array([dst.ptr(r) for r in range(n)])
    want = AK.f32_bits(AK.probe_expected(numel, seed))

    def call(st):
        assert L.fa_write_probe_f32(arr_, n, numel, seed, sp(st)) == OK, L.fa_last_error()

    def check(res, arr):
        h = res.out[0].view(np.uint32)
        nw = numel - numel % 4
        assert (h[:, GUARD:GUARD + nw] != AK.G32).all(), "the sentinel: the probe had not run"
        assert (h[:, GUARD:GUARD + nw] == want[None, :]).all()
        assert (h[:, :GUARD] == AK.G32).all() and (h[:, GUARD + nw:] == AK.G32).all(), "guards"

    return SimpleNamespace(call=call, inputs=[], outputs=[dst.t], check=check)


@case("read-probe", ["fa_read_probe_f32"], arrs="B")
def _read_probe():
    grid, numel = 3, 1024 * 4 + 3
    rng = np.random.default_rng(grid * 1000003 + numel)
    x = rng.integers(-8, 9, numel).astype(np.float32)
    nv = numel // 4
    owner = (np.arange(nv) // 256) % grid
    per_v = x[:4 * nv].astype(np.float64).reshape(nv, 4).sum(1)
    want = np.array([per_v[owner == k].sum() for k in range(grid)])
    marker = np.float32(-55.25)               # the sums accumulate onto it (exact: integers)
    src = AK.Guarded(numel, x)
    out = AK.Guarded(grid, np.full(grid, marker, np.float32))
    inputs = [SG.In(src.t)]

    def call(st):
        assert L.fa_read_probe_f32(src.ptr(), numel, out.ptr(), grid, sp(st)) == OK

    def check(res, arr):
        h = res.out[0].view(np.uint32)[0]
        got = h[GUARD:GUARD + grid].view(np.float32).astype(np.float64)
        assert (got != float(marker)).any(), "the sentinel: the probe had not run"
        assert np.array_equal(got, want + float(marker)), (got, want)
        assert (h[:GUARD] == AK.G32).all() and (h[GUARD + 4:] == AK.G32).all(), "guards"

    return SimpleNamespace(call=call, inputs=inputs, outputs=[out.t], check=check)


# ================================================================ the tests ====
@pytest.fixture(scope="module")
def side():
    """The side stream, after the power check in both arrangements."""
    torch.cuda.set_device(0)
    S = torch.cuda.Stream()
    for arr in "AB":
        SG.power_check(arr, S)
    yield S
    print(SG.report())


PARAMS = [(name, arr) for name in CASES for arr in CASES[name].arrs]


@pytest.mark.gpu
@pytest.mark.parametrize("name,arr", PARAMS, ids=[f"{n}-{a}" for n, a in PARAMS])
def test_stream_order(side, name, arr):
    k = CASES[name].build()
    torch.cuda.synchronize()
    res = SG.run(arr, side, k.call, k.inputs, k.outputs, name)
    k.check(res, arr)


# ====================================================== completeness (CPU) ====
EXCLUDED = {
    # include/fedagg_comm.h: these need a communicator and are pinned in
    # tests/test_gpu_stream_order_py.py; the guard below checks that the cases
    # named here are there
    "fa_shard_io": "a struct: the Native*Aggregator cases of test_gpu_stream_order_py.py (AGGS, "
                   "NativeAggregator for fa_reduce_multi among them) pass the side stream in it",
    "fa_mean_f32_multi": "test_gpu_stream_order_py.py::test_mean_f32_multi_on_a_side_stream",
    "fa_mean_f32_multi_ex": "test_gpu_stream_order_py.py::test_mean_f32_multi_on_a_side_stream",
}
PINNED_IN_PY = ['"NativeShardedAggregator"', '"NativeStripedAggregator"', '"NativeChainedAggregator"',
                '"NativeBlockedAggregator"', '"NativeAggregator"',
                'def test_mean_f32_multi_on_a_side_stream', '"fa_mean_f32_multi"',
                '"fa_mean_f32_multi_ex"', "a.step(stream=st.cuda_stream)"]


def _header(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", name)).read()
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def stream_entry_points():
    """Functions with a ``void *stream`` parameter and structs with a
    ``stream`` field, from both headers."""
    found = set()
    for h in ("fedagg.h", "fedagg_comm.h"):
        text = _header(h)
        for m in re.finditer(r"\b(\w+)\s*\(([^;{}()]*)\)\s*;", text):
            if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
                found.add(m.group(1))
        for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{([^}]*)\}", text):
            if re.search(r"\bstream\s*;", m.group(2)):
                found.add(m.group(1))
    return found


def test_every_stream_entry_point_is_pinned_or_excluded():
    found = stream_entry_points()
    assert {"fa_reduce", "fa_reduce_tab", "fa_prox_grad_elem", "fa_shard_io",
            "fa_mean_f32_multi_ex"} <= found, found          # the parser does parse
    assert len(found) >= 23, sorted(found)
    covered = {e for c in CASES.values() for e in c.entries}
    assert covered <= found, covered - found
    missing = found - covered - set(EXCLUDED)
    assert not missing, f"entry points with a stream and no stream-order case: {sorted(missing)}"
    assert not covered & set(EXCLUDED), "excluded and covered"
    for k, why in EXCLUDED.items():
        assert k in found and len(why) > 20, k
    py = open(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                           "test_gpu_stream_order_py.py")).read()
    for token in PINNED_IN_PY:
        assert token in py, f"EXCLUDED points at a case that is not there: {token}"
