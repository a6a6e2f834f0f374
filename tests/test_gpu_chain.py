"""GPU: chained segments of the cascade (fa_reduce_chain) — the exact form
of the client-sharded round.  Client groups reduced by
separate launches, each continuing the previous group's accumulator state in
slot order, give the single launch's bits; the layout's scalar columns
(ILP-4 tails, M==1, int64) are reduced over all clients' raw values, as the
multi-GPU round gathers them.  Reference order: train_feddct.py:42-50 /
train_fedavg.py:145-146 over the slots in list order."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_manifest
from feddct_amd import synth
from feddct_amd.layout import BucketLayout
from helpers import bits_equal, buckets_to_state, states_to_buckets
from oracle import torch_order as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib():
    from feddct_amd import _lib
    torch.cuda.set_device(DEV)
    return _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _plans(lib, layout):
    from feddct_amd.partition import layout_tiles
    _, tiles = layout_tiles(layout)
    vec, rest = tiles[tiles[:, 2] == 0], tiles[tiles[:, 2] != 0]
    mk = (lambda t: lib.Plan(None, layout.f32_numel, None, layout.i64_numel, 0, tiles=t)
          if len(t) else None)
    return mk(vec), mk(rest)


def chained(lib, layout, buckets, bounds, weights=None, inplace=True, flags=0):
    """Reduce ``buckets`` as the chained groups [bounds[g], bounds[g+1]);
    ``flags`` go to the finishing segment (and the scalar columns' reduce)."""
    vec, rest = _plans(lib, layout)
    n = len(buckets)
    plane = layout.f32_numel
    out32 = torch.full_like(buckets[0][0], np.nan)
    out64 = torch.full_like(buckets[0][1], -7)
    st = [torch.full((4 * plane,), np.nan, device=DEV) for _ in range(1 if inplace else 2)]
    w = None if weights is None else np.asarray(weights, np.float32)
    prev = None
    for g, (a, b) in enumerate(zip(bounds, bounds[1:])):
        last = b == n
        dst = None if last else st[g % len(st)]
        ch = lib.FaChain(a, n, prev.data_ptr() if prev is not None else None,
                         dst.data_ptr() if dst is not None else None, plane)
        wa = None if w is None else (ctypes.c_float * (b - a))(*map(float, w[a:b]))
        if vec is not None:
            lib.check(lib.lib.fa_reduce_chain(
                vec.handle, lib.ptr_array([x[0].data_ptr() for x in buckets[a:b]]), b - a, wa,
                ctypes.byref(ch), out32.data_ptr() if last else None, flags if last else 0,
                _stream()), "fa_reduce_chain")
        prev = dst
    if rest is not None:
        wall = None if w is None else (ctypes.c_float * n)(*map(float, w))
        lib.check(lib.lib.fa_reduce(rest.handle, lib.ptr_array([x[0].data_ptr() for x in buckets]),
                                    lib.ptr_array([x[1].data_ptr() for x in buckets]), n, wall,
                                    out32.data_ptr(), out64.data_ptr(), flags, _stream()), "tails")
    torch.cuda.synchronize()
    return out32, out64


def single(lib, layout, buckets, weights=None, flags=0):
    plan = lib.Plan(layout.segs32, layout.f32_numel, layout.segs64, layout.i64_numel)
    n = len(buckets)
    out32 = torch.full_like(buckets[0][0], np.nan)
    out64 = torch.full_like(buckets[0][1], -7)
    w = None if weights is None else (ctypes.c_float * n)(*map(float, weights))
    lib.check(lib.lib.fa_reduce(plan.handle, lib.ptr_array([x[0].data_ptr() for x in buckets]),
                                lib.ptr_array([x[1].data_ptr() for x in buckets]), n, w,
                                out32.data_ptr(), out64.data_ptr(), flags, _stream()), "fa_reduce")
    torch.cuda.synchronize()
    return out32, out64


MAN = {"keys": [{"key": f"k{j}", "shape": [m] if m else [], "dtype": "float32"}
                for j, m in enumerate([100, 4096, 33, 2048 + 8, 7, 0, 5000, 64, 1])]
       + [{"key": "nbt", "shape": [], "dtype": "int64"}]}


def _cuts(rng, n, groups):
    if groups >= n:
        return list(range(n + 1))
    c = sorted(rng.choice(np.arange(1, n), size=groups - 1, replace=False).tolist())
    return [0] + c + [n]


@pytest.mark.parametrize("n", [2, 5, 16, 20, 24, 33, 64, 100, 257, 300])
@pytest.mark.parametrize("groups", [2, 3, 8])
def test_chain_equals_one_launch(lib, n, groups):
    layout = BucketLayout.from_manifest(MAN)
    states = [synth.gen_state(MAN, i, synth.MODE_ADVERSARIAL) for i in range(n)]
    bk = states_to_buckets(layout, states, DEV)
    r32, r64 = single(lib, layout, bk)
    rng = np.random.default_rng(n * 10 + groups)
    for bounds in (_cuts(rng, n, groups), [0] + [b for b in (16, 32, 256) if b < n] + [n]):
        for inplace in (True, False):
            o32, o64 = chained(lib, layout, bk, bounds, inplace=inplace)
            for (k, a), (_, b) in zip(buckets_to_state(layout, o32, o64),
                                      buckets_to_state(layout, r32, r64)):
                assert bits_equal(a, b), (n, bounds, k)
    want = dict(O.aggregate_state(states))
    for k, v in buckets_to_state(layout, o32, o64):
        assert bits_equal(v, want[k]), k


def test_chain_weighted(lib):
    n = 20
    layout = BucketLayout.from_manifest(MAN)
    states = [synth.gen_state(MAN, i, synth.MODE_ADVERSARIAL) for i in range(n)]
    bk = states_to_buckets(layout, states, DEV)
    w = O.weights_from_sizes(np.arange(1, n + 1) * 7 + 3)
    r32, _ = single(lib, layout, bk, weights=w)
    o32, _ = chained(lib, layout, bk, [0, 7, 13, 20], weights=w)
    assert bits_equal(o32.cpu().numpy(), r32.cpu().numpy())


# ---- the deep cascade: n_total > 4096 (level 3, the fourth state plane) ----
# A reduced manifest that keeps every vector-tile shape the chain plan
# carries (a full 2048-float tile, partial ones, unaligned keys, a 0-d key,
# an int64 key) in ~2.3 k floats, so thousands of clients stay cheap.
DEEP_MAN = {"keys": [{"key": f"k{j}", "shape": [m] if m else [], "dtype": "float32"}
                     for j, m in enumerate([100, 2048 + 8, 33, 7, 0, 64, 1])]
            + [{"key": "nbt", "shape": [], "dtype": "int64"}]}
DEEP_MAX = 8193
_deep_cache = {}


def _deep_clients():
    """The first DEEP_MAX adversarial clients of DEEP_MAN, generated and
    uploaded once (client i's state depends on i alone, so every n_total
    takes a prefix): (layout, states, buckets)."""
    if "clients" not in _deep_cache:
        layout = BucketLayout.from_manifest(DEEP_MAN)
        states = [synth.gen_state(DEEP_MAN, i, synth.MODE_ADVERSARIAL) for i in range(DEEP_MAX)]
        row = -(-max(layout.f32_numel, 64) // 64) * 64
        f32 = np.zeros((DEEP_MAX, row), np.float32)
        i64 = np.zeros((DEEP_MAX, max(layout.i64_numel, 1)), np.int64)
        for i, st in enumerate(states):
            for k, v in st:
                s = layout.by_key[k]
                (i64 if s.kind == "i64" else f32)[i, s.offset:s.offset + s.numel] = \
                    np.asarray(v).reshape(-1)
        d32, d64 = torch.from_numpy(f32).to(DEV), torch.from_numpy(i64).to(DEV)
        _deep_cache["clients"] = (layout, states, [(d32[i], d64[i]) for i in range(DEEP_MAX)])
    return _deep_cache["clients"]


def _deep_reference(lib, n):
    """One launch over the first n clients and the oracle's state for them."""
    if n not in _deep_cache:
        layout, states, bk = _deep_clients()
        r32, r64 = single(lib, layout, bk[:n])
        _deep_cache[n] = (buckets_to_state(layout, r32, r64), dict(O.aggregate_state(states[:n])))
    return _deep_cache[n]


def _deep_bounds(n):
    rng = np.random.default_rng(n)
    raw = [[0, 4096, n], [0, 4095, 4097, n], [0, 4095, 4096, 4097, n],
           [0, 256, 4096 - 16, 4096 + 16, n], [0, 16, 4080, n], _cuts(rng, n, 8)]
    sets = []
    for r in raw:
        b = sorted({x for x in r if 0 <= x <= n})
        if len(b) > 2:          # a proper cut is left
            sets.append(b)
    return sets


@pytest.mark.parametrize("n", [4096, 4097, 4112, 8193])
def test_chain_deep_levels_equal_one_launch(lib, n):
    """Segments cut around row 4096 — at it (plane 3 alone is live: three
    planes hold +0 and are neither stored nor loaded), one row before and
    after it (DEEP kernels with a single local row), on block and
    256-multiples, and an 8-way random cut — give the one launch's bits and
    the oracle's, with NaN in every state plane the levels do not name."""
    layout, states, bk = _deep_clients()
    ref, want = _deep_reference(lib, n)
    sets = _deep_bounds(n)
    if n > 4096:
        assert [0, 4096, n] in sets and lib.lib.fa_chain_levels(4096, n) == 8
    for bounds in sets:
        for b in bounds:
            assert lib.lib.fa_chain_levels(b, n) == O.chain_levels(b, n), (b, n)
        for inplace in (True, False):
            o32, o64 = chained(lib, layout, bk[:n], bounds, inplace=inplace)
            for (k, a), (_, b) in zip(buckets_to_state(layout, o32, o64), ref):
                assert bits_equal(a, b), (n, bounds, inplace, k, "vs one launch")
                assert bits_equal(a, want[k]), (n, bounds, inplace, k, "vs oracle")


@pytest.mark.parametrize("bounds", [[0, 4096, 4097], [0, 100, 4095, 4097]])
def test_chain_deep_weighted(lib, bounds):
    n = 4097
    layout, states, bk = _deep_clients()
    w = O.weights_from_sizes(np.arange(1, n + 1) * 7 + 3)
    r32, r64 = single(lib, layout, bk[:n], weights=w)
    o32, o64 = chained(lib, layout, bk[:n], bounds, weights=w)
    ref = buckets_to_state(layout, r32, r64)
    for j, ((k, a), (_, b)) in enumerate(zip(buckets_to_state(layout, o32, o64), ref)):
        x = np.stack([s[j][1] for s in states[:n]])
        want = O.mean_i64_trunc(x) if x.dtype == np.int64 else O.weighted_sum0(x, w)
        assert bits_equal(a, b), (bounds, k, "vs one launch")
        assert bits_equal(a, want), (bounds, k, "vs oracle")


@pytest.mark.parametrize("n,bounds", [(20, [0, 7, 13, 20]), (300, [0, 16, 100, 256, 300]),
                                      (4097, [0, 100, 4095, 4096, 4097])])
def test_chain_sum_only(lib, n, bounds):
    """The finishing segment with FA_F_SUM_ONLY (the form the blocked round's
    continuation takes): the ordered sum without the division — fa_reduce's
    sum-only bits over all rows, and the oracle's cascade of the rows."""
    layout, states, bk = _deep_clients()
    r32, r64 = single(lib, layout, bk[:n], flags=lib.FA_F_SUM_ONLY)
    o32, o64 = chained(lib, layout, bk[:n], bounds, flags=lib.FA_F_SUM_ONLY)
    ref = buckets_to_state(layout, r32, r64)
    for j, ((k, a), (_, b)) in enumerate(zip(buckets_to_state(layout, o32, o64), ref)):
        assert bits_equal(a, b), (n, k, "vs one launch")
        x = np.stack([s[j][1] for s in states[:n]])
        if x.dtype == np.int64:
            continue            # int64 keys have no sum-only form
        assert bits_equal(a, O.torch_sum0(x)), (n, k, "vs oracle")
        body = O.body_len(x[0].size)
        if body:                # the chain's own columns: the plain cascade
            x2 = x.reshape(n, -1)
            assert bits_equal(a.reshape(-1)[:body], O.cascade([x2[i, :body] for i in range(n)]))


@pytest.mark.parametrize("n,a,b", [(300, 100, 256), (4097, 4000, 4096)])
def test_chain_sum_only_leaves_the_state_alone(lib, n, a, b):
    """A segment that does not finish stores the same state planes with
    FA_F_SUM_ONLY as without (the blocked round's K_PART / K_CONT pass the
    flag on every call)."""
    layout, _, bk = _deep_clients()
    vec, _ = _plans(lib, layout)
    plane = layout.f32_numel
    st_in = torch.full((4 * plane,), np.nan, device=DEV)
    ptrs = lambda lo, hi: lib.ptr_array([x[0].data_ptr() for x in bk[lo:hi]])
    ch = lib.FaChain(0, n, None, st_in.data_ptr(), plane)
    lib.check(lib.lib.fa_reduce_chain(vec.handle, ptrs(0, a), a, None, ctypes.byref(ch), None, 0,
                                      _stream()), "fa_reduce_chain")
    outs = []
    for flags in (0, lib.FA_F_SUM_ONLY):
        st = torch.full((4 * plane,), np.nan, device=DEV)
        ch = lib.FaChain(a, n, st_in.data_ptr(), st.data_ptr(), plane)
        lib.check(lib.lib.fa_reduce_chain(vec.handle, ptrs(a, b), b - a, None, ctypes.byref(ch),
                                          None, flags, _stream()), "fa_reduce_chain")
        torch.cuda.synchronize()
        outs.append(st.cpu().numpy())
    lev = O.chain_levels(b, n)
    assert lev and bits_equal(outs[0], outs[1])
    for l in range(4):          # and only the named planes were written at all
        p = outs[1][l * plane:(l + 1) * plane]
        assert np.isnan(p).all() if not lev & (1 << l) else not np.isnan(p).all(), l


@pytest.mark.parametrize("groups", [8, 3])
def test_chain_full_size_feddct_c100_digests(lib, golden, groups):
    """BASELINE config 5: 24 FedDCT slots (main + proxy in one bucket) as 8
    shards of 3 (the 8-GPU split) or 3 of 8, chained: both reference digests."""
    from feddct_amd.workload import joint_manifest, make_clients
    mm = load_manifest("wrnsl16_8_sf4_c100_main")
    pm = load_manifest("wrnsl16_8_sf4_c100_proxy")
    layout = BucketLayout.from_manifest(joint_manifest([mm, pm]))
    n = 24
    cl = make_clients(layout, [(mm, "0."), (pm, "1.")], range(n), DEV)
    bounds = list(range(0, n + 1, n // groups))
    o32, o64 = chained(lib, layout, cl, bounds)
    state = buckets_to_state(layout, o32, o64)
    for pf, lay in (("0.", "main"), ("1.", "proxy")):
        part = [(k[2:], v) for k, v in state if k.startswith(pf)]
        assert O.state_digest(part) == golden["digests"][f"feddct/wrnsl16_8_sf4_c100_{lay}/n{n}"]


def test_chain_full_size_fedavg_digest(lib, golden):
    """BASELINE config 2 as 2 ranks x 10 clients: the wrn16_8 N=20 digest."""
    from feddct_amd.workload import make_clients
    man = load_manifest("wrn16_8_c10")
    layout = BucketLayout.from_manifest(man)
    cl = make_clients(layout, man, range(20), DEV)
    o32, o64 = chained(lib, layout, cl, [0, 10, 20])
    assert (O.state_digest(buckets_to_state(layout, o32, o64))
            == golden["digests"]["fedavg/wrn16_8_c10/n20"])


def test_chain_errors(lib):
    layout = BucketLayout.from_manifest(MAN)
    full = lib.Plan(layout.segs32, layout.f32_numel, layout.segs64, layout.i64_numel)
    vec, _ = _plans(lib, layout)
    b = torch.zeros(4 * layout.f32_numel, device=DEV)
    ptrs = lib.ptr_array([b.data_ptr()] * 4)
    L = lib.lib

    def call(plan, n, ch, out=b.data_ptr()):
        return L.fa_reduce_chain(plan.handle, ptrs, n, None, ctypes.byref(ch), out, 0, None)
    P = layout.f32_numel
    assert call(full, 2, lib.FaChain(0, 4, None, b.data_ptr(), P)) == lib.FA_E_INVAL
    assert b"scalar tiles" in L.fa_last_error()
    assert call(vec, 2, lib.FaChain(2, 4, None, None, P)) == lib.FA_E_INVAL   # state_in missing
    assert call(vec, 2, lib.FaChain(0, 4, None, None, P)) == lib.FA_E_INVAL   # finish too early
    assert call(vec, 3, lib.FaChain(2, 4, b.data_ptr(), None, P)) == lib.FA_E_INVAL  # > n_total
    assert call(vec, 2, lib.FaChain(0, 4, None, b.data_ptr(), 10)) == lib.FA_E_INVAL  # plane
    assert call(vec, 1, lib.FaChain(0, lib.FA_MAX_CLIENTS + 1, None, b.data_ptr(), P)) == lib.FA_E_RANGE
