"""The chained multi-GPU round on fp16 / bf16 buckets, without a GPU: the new
symbols, the option-taking host entries of libfedagg_comm.so
(fa_describe_round_opts, fa_round_model_opts, fa_multi_select_layout_elem),
every rank's chained schedule replayed together on 16-bit buffers with fp32
state planes (tests/chain16.SimChain16), the cost model, and
feddct_amd/dist.py's ChainAggregator with its opt-in over the in-process
torch.distributed stand-in (tests/distloop.py) with an oracle backend.

Every comparison is bit for bit (two NaNs equal, round16.same16)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import chain16 as K
import feddct_amd.dist as D
import round16 as R
from conftest import ROOT, load_manifest
from distloop import LoopDist, run_ranks
from feddct_amd import _lib
from feddct_amd import comm as C
from feddct_amd.layout import BucketLayout
from feddct_amd.partition import chain_cut, layout_tiles
from oracle import torch_order as O

DTYPE_NAMES = ("float16", "bfloat16")
CHAINED, STRIPED = C.FA_MODE_CHAINED, C.FA_MODE_STRIPED
MODES = (C.FA_MODE_SHARDED, STRIPED, CHAINED, C.FA_MODE_BLOCKED)
HOLES = [0, 3, 0, 4, 5, 0, 8, 0]       # ranks without clients first, in the middle and last
PAD = _lib.FA_PLAN_GAPS_ARE_PADDING


# ------------------------------------------------------------------ symbols --
def test_the_new_entries_are_declared_exported_and_bound():
    """(fails on a tree without the feature)"""
    hdr = open(os.path.join(ROOT, "include", "fedagg.h")).read()
    assert re.search(r"\bint\s+fa_reduce_chain_elem\s*\(", hdr)
    assert "fa_reduce_chain_elem" in _lib.EXPORTS
    fn = _lib.lib.fa_reduce_chain_elem
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 8
    chdr = open(os.path.join(ROOT, "include", "fedagg_comm.h")).read()
    for name in ("fa_describe_round_opts", "fa_round_model_opts", "fa_multi_select_layout_elem"):
        assert name in C.COMM_EXPORTS and re.search(r"\bint\s+" + name + r"\s*\(", chdr), name
        assert getattr(C.lib(), name).argtypes
    assert C.FA_ROUND_CHAIN16 == int(re.search(r"#define\s+FA_ROUND_CHAIN16\s+(\d+)u", chdr).group(1))
    # no GPU needed to be refused: a NULL plan is fa_reduce_chain's refusal
    ch = _lib.FaChain(0, 2, None, None, 8)
    assert fn(None, None, 1, None, ctypes.byref(ch), None, 0, None) == _lib.FA_E_INVAL
    assert _lib.lib.fa_last_error().startswith(b"fa_reduce_chain: plan/chain is NULL")


# ------------------------------------------------- ropts == 0: the _elem entry --
def _describe(entry, lay, counts, rank, nchunks, root, weighted, mode, tail):
    """(rc, the ops' bytes or the message)."""
    n = ctypes.c_int()
    args = (mode, len(counts), rank, C._counts(counts), *C._layout_args(lay), nchunks, 0, PAD,
            root, weighted)
    rc = entry(*args, None, 0, ctypes.byref(n), *tail)
    if rc:
        return rc, _lib.lib.fa_last_error()
    arr = (C.FaXfer * max(1, n.value))()
    rc = entry(*args, arr, n.value, ctypes.byref(n), *tail)
    return rc, bytes(arr)[:n.value * ctypes.sizeof(C.FaXfer)]


def _model(entry, lay, counts, nchunks, root, weighted, mode, tail):
    out = C.FaRoundCost()
    rc = entry(mode, len(counts), C._counts(counts), *C._layout_args(lay), nchunks, 0, PAD, root,
               weighted, ctypes.byref(out), *tail)
    return (rc, _lib.lib.fa_last_error()) if rc else (rc, bytes(out))


@pytest.mark.parametrize("mode", MODES)
def test_no_option_is_the_elem_entry(mode):
    """The same ops, the same cost, the same refusals with the same messages
    (16-bit chained / weighted included), on 16-bit and fp32 layouts."""
    lib = C.lib()
    lays = [(R.layout_of(name, dt), R.ELEM[dt]) for name in ("A", "B", "raw")
            for dt in DTYPE_NAMES] + [(R.fp32_layout_of("B"), _lib.FA_ELEM_F32)]
    counts = [9, 8, 0, 7]
    refused = 0
    for lay, elem in lays:
        for weighted in (0, 1):
            for rank in (0, 2, 3):
                a = _describe(lib.fa_describe_round_elem, lay, counts, rank, 3, 1, weighted, mode,
                              (elem,))
                b = _describe(lib.fa_describe_round_opts, lay, counts, rank, 3, 1, weighted, mode,
                              (elem, 0))
                assert a == b, (elem, weighted, rank)
                refused += a[0] != 0
            a = _model(lib.fa_round_model_elem, lay, counts, 3, 1, weighted, mode, (elem,))
            b = _model(lib.fa_round_model_opts, lay, counts, 3, 1, weighted, mode, (elem, 0))
            assert a == b, (elem, weighted)
            if elem != _lib.FA_ELEM_F32 and (mode != STRIPED or weighted):
                assert a[0] == _lib.FA_E_INVAL
                assert (b"weighted" if mode == STRIPED else b"striped") in a[1]
                assert a[1].startswith(b"fa_round_model_elem:")
    assert refused or mode == STRIPED


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_the_option_is_the_chained_round_on_16_bits_only(dtype):
    lib = C.lib()
    l16, l32, el = R.layout_of("A", dtype), R.fp32_layout_of("A"), R.ELEM[dtype]
    bit = C.FA_ROUND_CHAIN16
    for mode in MODES:
        rc, msg = _describe(lib.fa_describe_round_opts, l16, [3, 2], 0, 2, 0, 0, mode, (el, bit))
        rm, mmsg = _model(lib.fa_round_model_opts, l16, [3, 2], 2, 0, 0, mode, (el, bit))
        if mode == CHAINED:
            assert rc == 0 and rm == 0
            continue
        assert rc == rm == _lib.FA_E_INVAL
        assert msg.startswith(b"fa_describe_round_opts:") and b"FA_MODE_CHAINED" in msg
        assert mmsg.startswith(b"fa_round_model_opts:")
    rc, msg = _describe(lib.fa_describe_round_opts, l32, [3, 2], 0, 2, 0, 0, CHAINED,
                        (_lib.FA_ELEM_F32, bit))
    assert rc == _lib.FA_E_INVAL and b"fp16 / bf16" in msg
    rc, msg = _describe(lib.fa_describe_round_opts, l16, [3, 2], 0, 2, 0, 0, CHAINED, (el, 6))
    assert rc == _lib.FA_E_INVAL and b"unknown round options" in msg
    with pytest.raises(ValueError, match="native 16-bit layout"):
        C.multi_select([3, 2], layout=l32, chain16=True)
    with pytest.raises(_lib.FedaggError, match="fa_multi_select_layout_elem"):
        C.multi_select([3, 2], layout=l16, chain16=True, exact=False)
    # without the bit a 16-bit bucket has the striped round alone; F32 is the fp32 entry
    m, k, us = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    out = (ctypes.byref(m), ctypes.byref(k), ctypes.byref(us))
    head = (2, C._counts([3, 2]), *C._layout_args(l16), PAD, 0)
    assert lib.fa_multi_select_layout_elem(*head, el, 0, *out) == 0 and m.value == STRIPED
    head32 = (2, C._counts([3, 2]), *C._layout_args(l32), PAD, 0)
    assert lib.fa_multi_select_layout_elem(*head32, _lib.FA_ELEM_F32, 0, *out) == 0
    assert (C.MODE_NAMES[m.value], k.value, us.value) == C.multi_select([3, 2], layout=l32,
                                                                        detail=True)
    assert lib.fa_multi_select_layout_elem(*head32, _lib.FA_ELEM_F32, bit, *out) == _lib.FA_E_INVAL


# ---------------------------------------------------------------- schedules --
def _scheds(lay, counts, nchunks, root, weighted=False):
    return [C.describe(CHAINED, lay, counts, r, nchunks=nchunks, root=root, weighted=weighted,
                       chain16=True) for r in range(len(counts))]


def _count_sets(W):
    sets = [D.shard_counts(n, W) for n in (5, 20, 300)]
    if W == 8:
        sets.append(HOLES)
    return sets


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
@pytest.mark.parametrize("name", R.LAYOUTS)
def test_chain16_schedules(name, dtype):
    """W = 1..8: the vector chunks are cut on multiples of 128 elements and
    cover exactly the layout's vector tiles, per ordered pair of ranks the
    sends match the receives in posting order, offset and count, and only the
    state planes fa_chain_levels names travel (between neighbours holding
    clients: the state after the sender's last row)."""
    lay = R.layout_of(name, dtype)
    _, tiles = layout_tiles(lay)
    vec = tiles[tiles[:, 2] == 0]
    for W in range(1, 9):
        for counts in _count_sets(W):
            n = sum(counts)
            first = [sum(counts[:r]) for r in range(W)]
            for nchunks in (1, 16):
                root = W - 1 if nchunks == 1 else -1
                sch = _scheds(lay, counts, nchunks, root)
                chunks = sorted({(x["offset"], x["count"]) for s in sch for x in s
                                 if x["op"] == "K_CHAIN"})
                assert len(chunks) <= nchunks and (len(chunks) > 0) == (len(vec) > 0)
                pos = 0
                for off, cnt in chunks:
                    assert off % 128 == 0 and off >= pos and cnt > 0, (W, counts, chunks)
                    pos = off + cnt
                for s0, c0, _ in vec:       # every vector tile inside one chunk
                    assert any(o <= s0 and s0 + c0 <= o + c for o, c in chunks), (W, s0)
                for a in range(W):
                    for b in range(W):
                        if a == b:
                            continue
                        sends = [(x["src"], x["src_index"] if x["src"] == "STATE" else -1,
                                  x["offset"], x["count"]) for x in sch[a]
                                 if x["op"] == "SEND" and x["peer"] == b]
                        recvs = [("STATE" if x["dst"] == "STATE" else "FIN",
                                  x["dst_index"] if x["dst"] == "STATE" else -1,
                                  x["offset"], x["count"]) for x in sch[b]
                                 if x["op"] == "RECV" and x["peer"] == a]
                        assert [(("STATE" if s[0] == "STATE" else "FIN"),) + s[1:]
                                for s in sends] == recvs, (W, counts, a, b)
                        planes = {s[1] for s in sends if s[0] == "STATE"}
                        if planes:
                            assert b == a + 1
                            lev = O.chain_levels(first[a] + counts[a], n)
                            assert planes == {l for l in range(4) if lev & (1 << l)}, (W, a, lev)
                for r, s in enumerate(sch):   # a chain kernel covers the rank's own rows
                    for x in s:
                        if x["op"] == "K_CHAIN":
                            assert (x["row0"], x["nrows"]) == (first[r], counts[r]) and counts[r] > 0


CASES = [  # layout, counts, nchunks, root, weighted
    ("A", [20], 16, 0, False), ("A", [3, 2], 1, -1, False), ("A", [10, 10], 16, 1, True),
    ("B", [7, 13], 16, 0, False), ("B", [100, 100, 100], 16, -1, False),
    ("B", [9, 0, 11], 1, 0, True), ("B", HOLES, 16, 6, False), ("B", HOLES, 1, 0, True),
    ("C", [260, 40], 16, 1, False), ("C", [1, 1, 1, 1, 1, 0, 0, 0], 1, -1, True),
    ("raw", [0, 3, 2], 16, 1, False), ("raw", D.shard_counts(300, 8), 16, 3, False),
    ("raw", [4, 1], 1, 0, True), ("A", D.shard_counts(5, 8), 16, -1, False)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)).replace(" ", ""))
def test_replayed_chain16_round_is_the_single_bucket_result(case):
    """All ranks' schedules replayed: every result rank holds
    round16.expected16 (weighted: the weighted expectation) and the int64
    means; the other ranks keep their fill."""
    name, counts, nchunks, root, weighted = case
    W, n = len(counts), sum(counts)
    for dtype in DTYPE_NAMES:
        lay = R.layout_of(name, dtype)
        bits, i64 = R.clients16(name, dtype, n, seed=W + nchunks)
        w = O.weights_from_sizes(np.arange(1, n + 1) * 5 + 2) if weighted else None
        exp, inside, e64 = (R.expected16(lay, dtype, bits, i64) if w is None
                            else K.expected16w(lay, dtype, bits, w, i64))
        _, tiles = layout_tiles(lay)
        sim = K.SimChain16(lay, dtype, tiles, counts, list(bits),
                           list(i64[:, :max(1, lay.i64_numel)]), weights=w)
        bufs = sim.run(_scheds(lay, counts, nchunks, root, weighted))
        for r in range(W):
            out = bufs[r]["OUT"]
            if root < 0 or root == r:
                assert R.same16(out[inside], exp[inside], dtype), (case, dtype, r)
                if lay.i64_numel:
                    assert np.array_equal(bufs[r]["OUT64"][:lay.i64_numel], e64), (case, dtype, r)
            else:
                assert (out == R.FILL16).all() and (bufs[r]["OUT64"] == -7).all(), (case, r)


def test_weighted_chain16_gathers_the_weights_once():
    """One all-gather of nmax fp32 weights beside the scalar columns', before
    K_TAILS, no K_SCALE; none without scalar columns (layout C) or weights."""
    for name, want in (("A", 1), ("C", 0)):
        lay = R.layout_of(name, "bfloat16")
        for weighted in (False, True):
            for s in _scheds(lay, [3, 0, 4], 4, 2, weighted):
                g = [x for x in s if x["op"] == "ALLGATHER" and x["src_index"] == 2]
                assert len(g) == (want if weighted else 0)
                assert not [x for x in s if x["op"] == "K_SCALE"]
                for x in g:
                    assert (x["src"], x["dst"], x["dst_index"], x["count"]) == ("STACK", "GATHER", 2, 4)
                    tails = [y for y in s if y["op"] == "K_TAILS"]
                    assert all(y["step"] > x["step"] for y in tails)


# -------------------------------------------------------------------- model --
@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_model_on_layout_c(dtype):
    """Layout C (vector tiles only, every key a multiple of 128 elements): the
    cuts coincide with fp32's.  With the result on the finisher only the fp32
    planes cross a link: the same link bytes as the fp32 chained round.  The
    busiest rank's HBM bytes differ by exactly the clients' halved bytes (and
    the halved result row), and the modelled time is no higher."""
    l16, l32 = R.layout_of("C", dtype), R.fp32_layout_of("C")
    V = l16.f32_numel
    assert V == l32.f32_numel == 2048 + 4096 and not l16.i64_numel
    for k, nchunks in ((3, 1), (10, 4), (20, 16), (150, 8)):
        counts = [k, k]
        a = C.round_model(CHAINED, l32, counts, nchunks, root=1)
        b = C.round_model(CHAINED, l16, counts, nchunks, root=1, chain16=True)
        assert a["link_bytes_max"] == b["link_bytes_max"] > 0, (k, a, b)
        assert (a["groups"], a["steps"]) == (b["groups"], b["steps"])
        # rank 1: k client rows and the result row at 2 B instead of 4
        assert a["hbm_bytes_max"] - b["hbm_bytes_max"] == (k + 1) * 2 * V, (k, a, b)
        assert b["model_us"] <= a["model_us"]
        for x, y in zip(C.describe(CHAINED, l32, counts, 1, nchunks=nchunks, root=1),
                        C.describe(CHAINED, l16, counts, 1, nchunks=nchunks, root=1, chain16=True)):
            assert x == y
    one32 = C.round_model(CHAINED, l32, [5], 1, root=0)
    one16 = C.round_model(CHAINED, l16, [5], 1, root=0, chain16=True)
    assert one16["hbm_bytes_max"] * 2 == one32["hbm_bytes_max"]


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_model_is_no_slower_than_fp32_chained(dtype):
    for name in ("A", "B"):
        l16, l32 = R.layout_of(name, dtype), R.fp32_layout_of(name)
        for counts in ([20, 20], [7, 13], D.shard_counts(300, 8), HOLES):
            for weighted in (False, True):
                a = C.round_model(CHAINED, l32, counts, 8, root=len(counts) - 1, weighted=weighted)
                b = C.round_model(CHAINED, l16, counts, 8, root=len(counts) - 1,
                                  weighted=weighted, chain16=True)
                assert b["model_us"] <= a["model_us"], (name, counts, weighted, a, b)


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_wrn16_8_picks(dtype):
    """The model's picks on wrn16_8 in 16 bits (its constants, not
    measurements): chained at 2 ranks x 20 clients — below the fp32 chained
    round of the same counts, which the striped 16-bit round is not — and
    striped at 8 ranks holding 20 clients in all.  Without the option: striped."""
    man = load_manifest("wrn16_8_c10")
    l32 = BucketLayout.from_manifest(man)
    l16 = BucketLayout([(e["key"], e["shape"], e["dtype"] if e["dtype"] == "int64" else dtype)
                        for e in man["keys"]], native16=True)
    form, nch, us = C.multi_select([20, 20], layout=l16, chain16=True, detail=True)
    f32 = C.multi_select([20, 20], layout=l32, detail=True)
    striped = min(C.round_model(STRIPED, l16, [20, 20], c, root=1)["model_us"] for c in (1, 2, 4, 8))
    assert form == "chained" and f32[0] == "chained" and us < f32[2] < striped, (us, f32, striped)
    assert us == C.round_model(CHAINED, l16, [20, 20], nch, root=1, chain16=True)["model_us"]
    assert C.multi_select(D.shard_counts(20, 8), layout=l16, chain16=True) == "striped"
    assert D.exact_form([20, 20], l16) == "striped"
    assert D.exact_form([20, 20], l16, chain16=True) == "chained"
    assert C.multi_select([20], layout=l16, chain16=True) == "chained"


# ------------------------------------------------ dist.py's ChainAggregator --
def _out16(lay, dtype):
    return (R.as_tensor(np.full(lay.f32_numel, R.FILL16, np.uint16), dtype),
            torch.full((max(1, lay.i64_numel),), -7, dtype=torch.int64))


DIST = [  # layout, counts, final, root, nchunks, weighted
    ("A", [20], "reduce", 0, 3, False), ("B", [5], "allreduce", 0, 16, True),
    ("A", [7, 13], "reduce", 0, 3, False), ("B", [7, 13], "allreduce", 0, 16, True),
    ("raw", [0, 3, 2], "reduce", 0, 3, False), ("B", [9, 0, 11], "reduce", 1, 16, True),
    ("C", [100, 100, 100], "allreduce", 0, 3, False),
    ("B", HOLES, "reduce", 3, 16, False), ("raw", HOLES, "reduce", 0, 1, True),
    ("A", [1, 1, 1, 1, 1, 0, 0, 0], "allreduce", 0, 3, False)]


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
@pytest.mark.parametrize("name,counts,final,root,nchunks,weighted", DIST)
def test_dist_chain16_oracle_backend(monkeypatch, name, counts, final, root, nchunks, weighted,
                                     dtype):
    """W = 1, 2, 3, 8; two rounds of fresh data on one aggregator; root on a
    rank that is not the finisher and on one that holds no clients."""
    W, n = len(counts), sum(counts)
    monkeypatch.setattr(D, "dist", LoopDist(W, timeout=60.0))
    lay = R.layout_of(name, dtype)
    chunks, compact, _, _ = chain_cut(lay, nchunks)
    rounds = [R.clients16(name, dtype, n, seed=31 + k) for k in range(2)]
    w = O.weights_from_sizes(np.arange(1, n + 1) * 3 + 2) if weighted else None

    def fn(rank):
        a = sum(counts[:rank])
        out32, out64 = _out16(lay, dtype)
        agg = D.ChainAggregator(lay, n, out32, out64, final=final, root=root, nchunks=nchunks,
                                counts=counts, native16=True,
                                backend=K.OracleChainBackend16(lay, dtype, chunks, compact))
        assert agg.state.dtype == torch.float32 and agg.stack32.dtype == lay.float_dtype
        assert agg.gather32.dtype == lay.float_dtype
        assert agg.fin is None or agg.fin.dtype == lay.float_dtype
        res = []
        for bits, i64 in rounds:
            out32.copy_(_out16(lay, dtype)[0])
            out64.fill_(-7)
            loc = [R.as_tensor(bits[s], dtype) for s in range(a, a + counts[rank])]
            agg.step(loc, [torch.from_numpy(i64[s].copy()) for s in range(a, a + counts[rank])],
                     None if w is None else w[a:a + counts[rank]])
            same = all(np.array_equal(R.bits_of(t), bits[a + j]) for j, t in enumerate(loc))
            res.append((R.bits_of(out32).copy(), out64.numpy().copy(), same))
        return res

    res = run_ranks(W, fn)
    roots = set(range(W)) if final == "allreduce" else {root}
    for k, (bits, i64) in enumerate(rounds):
        exp, inside, e64 = (R.expected16(lay, dtype, bits, i64) if w is None
                            else K.expected16w(lay, dtype, bits, w, i64))
        for r in range(W):
            o16, o64, same = res[r][k]
            assert same, (r, k, "client buckets changed")
            if r not in roots:
                assert (o16 == R.FILL16).all() and (o64 == -7).all(), (r, k)
                continue
            assert R.same16(o16[inside], exp[inside], dtype), (r, k)
            if lay.i64_numel:
                assert np.array_equal(o64[:lay.i64_numel], e64), (r, k)


def test_pinned_refusals_without_the_opt_in(monkeypatch):
    monkeypatch.setattr(D, "dist", LoopDist(1, timeout=10.0))
    lay = R.layout_of("A", "bfloat16")
    out32, out64 = _out16(lay, "bfloat16")

    def fn(rank):
        with pytest.raises(ValueError, match="striped round only"):
            D.ChainAggregator(lay, 2, out32, out64)
        with pytest.raises(ValueError, match="striped round only"):
            D.ShardedAggregator(lay, [], [], 2, out32, out64)
        loc = [R.as_tensor(np.zeros(lay.f32_numel, np.uint16), "bfloat16") for _ in range(2)]
        l64 = [torch.zeros(max(1, lay.i64_numel), dtype=torch.int64) for _ in range(2)]
        with pytest.raises(ValueError, match="weighted rounds on 16-bit buckets"):
            D.Aggregator(lay, loc, l64, 2, out32, out64, weights=[0.5, 0.5], native=False)
        agg = D.Aggregator(lay, loc, l64, 2, out32, out64, native=False,
                           stripe_backend=R.OracleStripeBackend16(lay, "bfloat16"))
        assert agg.form == "striped/torch.distributed"
        assert D.exact_form([2], lay) == "striped"
        # with the opt-in: an fp32 result bucket, a bucket of another dtype
        with pytest.raises(TypeError, match="result bucket"):
            D.ChainAggregator(lay, 2, torch.zeros(lay.f32_numel), out64, native16=True)
        chunks, compact, _, _ = chain_cut(lay, 2)
        c = D.ChainAggregator(lay, 2, out32, out64, native16=True, nchunks=2,
                              backend=K.OracleChainBackend16(lay, "bfloat16", chunks, compact))
        with pytest.raises(TypeError, match="bucket on a native"):
            c.step([loc[0], loc[1].float()], l64)
        assert (R.bits_of(out32) == R.FILL16).all()
        # the Aggregator's opt-in: chained with weights, and where the model picks it
        be = K.OracleChainBackend16(lay, "bfloat16", *chain_cut(lay, 16)[:2])
        agg = D.Aggregator(lay, loc, l64, 2, out32, out64, weights=[0.5, 0.5], native=False,
                           chain16=True, backend=be)
        assert agg.form == "chained/torch.distributed"
        agg.step()
        assert (R.bits_of(out32)[:8] == 0).all()
        agg = D.Aggregator(lay, loc, l64, 2, out32, out64, native=False, chain16=True, backend=be)
        assert agg.form == "chained/torch.distributed"      # one rank: the chain is one launch
        return True

    assert run_ranks(1, fn) == [True]
