"""GPU parity: the HIP kernels (through the C ABI and through the drop-in
shim) against the oracle and the reference's own outputs.  Bit-exact for
every fp32 and int64 key (NaN positions must match; payloads are free)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_manifest
from feddct_amd import synth
from feddct_amd.layout import BucketLayout
from helpers import StateModule, bits_equal, buckets_to_state, states_to_buckets
from oracle import torch_order as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib():
    from feddct_amd import _lib
    torch.cuda.set_device(DEV)
    return _lib


def _reduce(lib, layout, buckets, weights=None, flags=0, tile_elems=0, out_pad=None):
    plan = lib.Plan(layout.segs32, layout.f32_numel, layout.segs64, layout.i64_numel,
                    tile_elems=tile_elems)
    n = len(buckets)
    out32 = torch.full_like(buckets[0][0], np.nan if out_pad is None else out_pad)
    out64 = torch.full_like(buckets[0][1], -7)
    w = None if weights is None else (ctypes.c_float * n)(*[float(x) for x in weights])
    stream = torch.cuda.current_stream().cuda_stream
    lib.check(lib.lib.fa_reduce(plan.handle, lib.ptr_array([b[0].data_ptr() for b in buckets]),
                                lib.ptr_array([b[1].data_ptr() for b in buckets]), n, w,
                                out32.data_ptr(), out64.data_ptr(), flags,
                                ctypes.c_void_p(stream)), "fa_reduce")
    torch.cuda.synchronize()
    return out32, out64


def _rand_manifest(rng, sizes):
    keys = [{"key": f"k{j}", "shape": [int(m)] if m != 0 else [], "dtype": "float32"}
            for j, m in enumerate(sizes)]
    keys.append({"key": "nbt", "shape": [], "dtype": "int64"})
    return {"keys": keys}


SIZES = [0, 2, 3, 4, 5, 7, 8, 9, 16, 31, 32, 33, 63, 64, 65, 100, 432, 1000, 2047, 2048, 2049,
         4097, 5120, 9000]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 20, 24, 31, 32, 33, 48, 64,
                               100, 127, 128, 129, 255, 256, 300])
@pytest.mark.parametrize("mode", [synth.MODE_REALISTIC, synth.MODE_ADVERSARIAL])
def test_reduce_matches_oracle(lib, n, mode):
    man = _rand_manifest(np.random.default_rng(n), SIZES)
    layout = BucketLayout.from_manifest(man)
    states = [synth.gen_state(man, i, mode) for i in range(n)]
    out32, out64 = _reduce(lib, layout, states_to_buckets(layout, states, DEV))
    got = buckets_to_state(layout, out32, out64)
    for (k, want), (k2, g) in zip(O.aggregate_state(states), got):
        assert k == k2 and bits_equal(g, want), (n, mode, k)


@pytest.mark.parametrize("n", [511, 512, 1000, 4095, 4096, 4097, 8193, 65536])
def test_many_clients_up_to_the_maximum(lib, n):
    """Up to FA_MAX_CLIENTS = 2^16: the device pointer table, the cascade's
    third and fourth levels (promotions after 16^2 and 16^3 = 4096 rows; l3
    accumulates every 4096-row block from there on) and every column rule,
    against the oracle and torch itself.  torch runs single-threaded here:
    with N*M >= 32768 its column chunking across threads can move a tensor's
    last few tail columns to another order; the engine defines
    the single-thread order, which is what torch produces for the reference's
    layouts."""
    sizes = [0, 1, 5, 33, 100, 1060] if n <= 8193 else [0, 1, 5, 33, 260]
    man = _rand_manifest(np.random.default_rng(n), sizes)
    layout = BucketLayout.from_manifest(man)
    states = [synth.gen_state(man, i, synth.MODE_ADVERSARIAL) for i in range(n)]
    out32, out64 = _reduce(lib, layout, states_to_buckets(layout, states, DEV))
    got = buckets_to_state(layout, out32, out64)
    for j, ((k, want), (k2, g)) in enumerate(zip(O.aggregate_state(states), got)):
        assert k == k2 and bits_equal(g, want), (n, k)
        x = np.stack([s[j][1] for s in states])
        if x.dtype == np.float32:
            nthr = torch.get_num_threads()
            torch.set_num_threads(1)
            try:
                ref = torch.from_numpy(x).mean(0).numpy()
            finally:
                torch.set_num_threads(nthr)
            assert bits_equal(g, ref), (n, k, "vs torch")


def test_weighted_many_clients(lib):
    n = 1000
    man = _rand_manifest(None, [1, 7, 100, 2049])
    layout = BucketLayout.from_manifest(man)
    states = [synth.gen_state(man, i, synth.MODE_ADVERSARIAL) for i in range(n)]
    w = O.weights_from_sizes(np.arange(1, n + 1) * 13)
    out32, out64 = _reduce(lib, layout, states_to_buckets(layout, states, DEV), weights=w)
    got = dict(buckets_to_state(layout, out32, out64))
    for j, (k, _) in enumerate(states[0]):
        x = np.stack([s[j][1] for s in states])
        want = O.mean_i64_trunc(x) if x.dtype == np.int64 else O.weighted_sum0(x, w)
        assert bits_equal(got[k], want), k


@pytest.mark.parametrize("n", [1, 3, 256, 257, 600])
def test_broadcast_f32(lib, n):
    """fa_broadcast_f32 (the stand-alone global -> clients copy): every
    destination gets every element, ragged tail included; more than 256
    destinations take consecutive launches."""
    numel = 1000 * 4 + 3
    src = torch.randn(numel, device=DEV)
    dst = [torch.full((numel + 5,), -1.0, device=DEV) for _ in range(n)]
    ptrs = (ctypes.c_void_p * n)(*[d.data_ptr() for d in dst])
    stream = torch.cuda.current_stream().cuda_stream
    lib.check(lib.lib.fa_broadcast_f32(ctypes.c_void_p(src.data_ptr()), ptrs, n, numel,
                                       ctypes.c_void_p(stream)), "fa_broadcast_f32")
    torch.cuda.synchronize()
    for d in dst:
        assert torch.equal(d[:numel], src)
        assert bool((d[numel:] == -1.0).all())


def test_too_many_clients_is_refused(lib):
    man = _rand_manifest(None, [4])
    layout = BucketLayout.from_manifest(man)
    plan = lib.Plan(layout.segs32, layout.f32_numel, layout.segs64, layout.i64_numel)
    n = lib.FA_MAX_CLIENTS + 1
    b = torch.zeros(64, device=DEV)
    rc = lib.lib.fa_reduce(plan.handle, lib.ptr_array([b.data_ptr()] * n), None, n, None,
                           b.data_ptr(), None, 0, None)
    assert rc == lib.FA_E_RANGE


@pytest.mark.parametrize("tile_elems", [1024, 2048, 4096])
def test_tile_sizes_bit_exact(lib, tile_elems):
    n = 20
    man = _rand_manifest(None, [8192 + 32, 4096, 12345, 1])
    layout = BucketLayout.from_manifest(man)
    states = [synth.gen_state(man, i, synth.MODE_ADVERSARIAL) for i in range(n)]
    out32, out64 = _reduce(lib, layout, states_to_buckets(layout, states, DEV),
                           tile_elems=tile_elems)
    for (k, want), (_, g) in zip(O.aggregate_state(states),
                                 buckets_to_state(layout, out32, out64)):
        assert bits_equal(g, want), k


def test_special_values_and_subnormals(lib):
    n, M = 17, 300
    rng = np.random.default_rng(11)
    x = rng.standard_normal((n, M)).astype(np.float32)
    x[:, 0] = -0.0
    x[:, 1] = np.float32(1e-45) * rng.integers(-5, 5, n)   # subnormals
    x[3, 2] = np.inf
    x[5, 3] = np.nan
    x[:, 4] = np.float32(3e38)                             # overflow to inf
    x[:, 5] = np.float32(1e-40)
    man = {"keys": [{"key": "t", "shape": [M], "dtype": "float32"}]}
    layout = BucketLayout.from_manifest(man)
    states = [[("t", x[i])] for i in range(n)]
    out32, _ = _reduce(lib, layout, states_to_buckets(layout, states, DEV))
    got = buckets_to_state(layout, out32, torch.zeros(1, dtype=torch.int64))[0][1]
    want = O.torch_mean0(x)
    assert bits_equal(got, want)
    ref = torch.from_numpy(x).mean(0).numpy()
    assert bits_equal(got, ref)
    assert got.view(np.uint32)[0] == 0


@pytest.mark.parametrize("n", [3, 20, 200])
def test_weighted_matches_oracle(lib, n):
    man = _rand_manifest(None, SIZES)
    layout = BucketLayout.from_manifest(man)
    states = [synth.gen_state(man, i, synth.MODE_ADVERSARIAL) for i in range(n)]
    w = O.weights_from_sizes(np.arange(1, n + 1) * 37)
    out32, out64 = _reduce(lib, layout, states_to_buckets(layout, states, DEV), weights=w)
    got = dict(buckets_to_state(layout, out32, out64))
    for j, (k, _) in enumerate(states[0]):
        x = np.stack([s[j][1] for s in states])
        want = O.mean_i64_trunc(x) if x.dtype == np.int64 else O.weighted_sum0(x, w)
        assert bits_equal(got[k], want), k


def test_sum_only_and_bcast_flags(lib):
    from feddct_amd._lib import FA_F_BCAST, FA_F_SUM_ONLY
    n = 9
    man = _rand_manifest(None, [100, 4096, 7, 1])
    layout = BucketLayout.from_manifest(man)
    states = [synth.gen_state(man, i, synth.MODE_ADVERSARIAL) for i in range(n)]
    bk = states_to_buckets(layout, states, DEV)
    out32, _ = _reduce(lib, layout, bk, flags=FA_F_SUM_ONLY)
    got = dict(buckets_to_state(layout, out32, torch.zeros(1, dtype=torch.int64)))
    for j, (k, _) in enumerate(states[0]):
        x = np.stack([s[j][1] for s in states])
        if x.dtype == np.float32:
            assert bits_equal(got[k], O.torch_sum0(x)), k
    bk = states_to_buckets(layout, states, DEV)
    out32, out64 = _reduce(lib, layout, bk, flags=FA_F_BCAST)
    want = buckets_to_state(layout, out32, out64)
    for f32, i64 in bk:
        for (k, a), (_, b) in zip(buckets_to_state(layout, f32, i64), want):
            assert bits_equal(a, b), k


@pytest.mark.parametrize("which", ["middle", "head", "tail", "i64_subset"])
def test_bcast_of_a_partial_plan_leaves_other_keys_alone(lib, which):
    """FA_F_BCAST on a gap-padded plan over SOME of a layout's
    keys (a column chunk) must write only that plan's keys into the clients;
    the flat bucket copy is for plans that cover the whole bucket."""
    from feddct_amd._lib import FA_F_BCAST
    n = 5
    man = _rand_manifest(None, [100, 4096, 7, 3000, 1, 64])
    man["keys"].append({"key": "nbt2", "shape": [], "dtype": "int64"})
    layout = BucketLayout.from_manifest(man)
    states = [synth.gen_state(man, i, synth.MODE_ADVERSARIAL) for i in range(n)]
    bk = states_to_buckets(layout, states, DEV)
    before = [(f.clone(), i.clone()) for f, i in bk]
    s32, s64 = layout.segs32, layout.segs64
    own = {"middle": [0, 2, 4, 5], "head": [0, 1, 2], "tail": [3, 4, 5]}.get(which)
    segs32 = s32 if own is None else s32[own]
    segs64 = s64[:1] if which == "i64_subset" else s64
    plan = lib.Plan(segs32, layout.f32_numel, segs64, layout.i64_numel)
    out32 = torch.zeros_like(bk[0][0])
    out64 = torch.zeros_like(bk[0][1])
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(lib.lib.fa_reduce(plan.handle, lib.ptr_array([b[0].data_ptr() for b in bk]),
                                lib.ptr_array([b[1].data_ptr() for b in bk]), n, None,
                                out32.data_ptr(), out64.data_ptr(), FA_F_BCAST, s))
    torch.cuda.synchronize()
    mine32 = {(int(o), int(m)) for o, m in segs32}
    mine64 = {(int(o), int(m)) for o, m in segs64}
    for (f, i), (f0, i0) in zip(bk, before):
        for o, m in s32:
            want = out32 if (int(o), int(m)) in mine32 else f0
            assert torch.equal(f[o:o + m], want[o:o + m]), (which, o)
        for o, m in s64:
            want = out64 if (int(o), int(m)) in mine64 else i0
            assert torch.equal(i[o:o + m], want[o:o + m]), (which, o)


@pytest.mark.parametrize("n", [1, 7, 20, 21, 24, 25, 49, 300])
@pytest.mark.parametrize("form", ["flat", "table", "tgpu"])
def test_broadcast_forms_and_bcast_only(lib, n, form):
    """Every broadcast form writes the global state into every client —
    FA_F_BCAST after the reduce and FA_F_BCAST_ONLY alone (the reference's
    initial sync, train_fedavg.py:244-250): the flat copy (gap-padded plans),
    client groups per tile (plans without gap padding: only segments are
    written) and the torch-GPU-order table; client counts that leave a short
    last group of <= 24 and part counts that are not a multiple of 8."""
    from feddct_amd._lib import FA_F_BCAST, FA_F_BCAST_ONLY
    man = _rand_manifest(None, [100, 4096, 7, 3000, 1, 64, 20000])
    layout = BucketLayout.from_manifest(man)
    states = [synth.gen_state(man, i % 9, synth.MODE_ADVERSARIAL) for i in range(n)]
    fl = 0 if form == "table" else lib.FA_PLAN_GAPS_ARE_PADDING
    kw = dict(order=lib.FA_ORDER_TORCH_GPU, n=n) if form == "tgpu" else {}
    if form == "tgpu" and not 2 <= n <= 128:
        pytest.skip("the torch-GPU order: N >= 2, and no row split past 16 warps (N=300 "
                    "splits the 7-element key 32 ways)")
    plan = lib.Plan(layout.segs32, layout.f32_numel, layout.segs64, layout.i64_numel,
                    flags=fl, **kw)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for flag in (FA_F_BCAST, FA_F_BCAST_ONLY):
        bk = states_to_buckets(layout, states, DEV)
        g32 = torch.randn_like(bk[0][0])
        g64 = torch.randint_like(bk[0][1], -1000, 1000)
        lib.check(lib.lib.fa_reduce(plan.handle, lib.ptr_array([b[0].data_ptr() for b in bk]),
                                    lib.ptr_array([b[1].data_ptr() for b in bk]), n, None,
                                    g32.data_ptr(), g64.data_ptr(), flag, s))
        torch.cuda.synchronize()
        for f, i in bk:
            for o, m in layout.segs32:
                assert torch.equal(f[o:o + m].view(torch.int32),
                                   g32[o:o + m].view(torch.int32)), (form, flag, o)
            assert torch.equal(i[:layout.i64_numel], g64[:layout.i64_numel]), (form, flag)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 15, 16, 20])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("tile", [0, 1024, 4096])
def test_round_small_n_every_tile_width(lib, n, weighted, tile):
    """FA_F_BCAST rounds around the 8- / 16-client kernel boundary: the
    global is the oracle's bits and every client's segments equal it; every
    tile width (U = 1, 2, 4), weighted or not, packed scalar columns and
    int64 keys included.  (r05 measured a one-launch form of these rounds —
    slower, DESIGN §4.2 item 5 — and kept reduce + broadcast.)"""
    man = _rand_manifest(None, [100, 4096, 7, 3000, 1, 64, 20000, 3, 9000])
    layout = BucketLayout.from_manifest(man)
    states = [synth.gen_state(man, i, synth.MODE_ADVERSARIAL) for i in range(n)]
    bk = states_to_buckets(layout, states, DEV)
    w = O.weights_from_sizes(np.arange(1, n + 1) * 7 + 3) if weighted else None
    plan = lib.Plan(layout.segs32, layout.f32_numel, layout.segs64, layout.i64_numel,
                    tile_elems=tile, flags=lib.FA_PLAN_GAPS_ARE_PADDING)
    o32 = torch.full_like(bk[0][0], np.nan)
    o64 = torch.full_like(bk[0][1], -7)
    wa = None if w is None else (ctypes.c_float * n)(*[float(x) for x in w])
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(lib.lib.fa_reduce(plan.handle, lib.ptr_array([b[0].data_ptr() for b in bk]),
                                lib.ptr_array([b[1].data_ptr() for b in bk]), n, wa,
                                o32.data_ptr(), o64.data_ptr(), lib.FA_F_BCAST, s))
    torch.cuda.synchronize()
    if w is None:
        want = O.aggregate_state(states)
    else:
        want = []
        for j, (k, v0) in enumerate(states[0]):
            x = np.stack([np.asarray(st[j][1]) for st in states])
            want.append((k, O.mean_i64_trunc(x) if x.dtype == np.int64 else O.weighted_sum0(x, w)))
    for (k, v), (_, g) in zip(want, buckets_to_state(layout, o32, o64)):
        assert bits_equal(g, v), (n, weighted, tile, k)
    for f, i in bk:
        for o, m in layout.segs32:
            assert torch.equal(f[o:o + m].view(torch.int32), o32[o:o + m].view(torch.int32)), o
        assert torch.equal(i[:layout.i64_numel], o64[:layout.i64_numel])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [2, 5, 7, 8, 16, 17, 20, 31, 33, 48, 63, 64])
def test_ragged_table_batch_form(lib, n, weighted):
    """A ragged layout (tiles past tensor ends, packed scalar columns, int64
    keys) on the plain table (FA_PLAN_TUNE_NO_BALANCE), against the oracle
    bit for bit, mean and round.  This launch is too short for the client
    loop (pipe_rule: three rounds of resident workgroups), so every tile takes
    the batch form — asserted; the client loop's own test is
    test_client_loop_instances_on_a_long_launch."""
    man = _rand_manifest(None, [100, 4096, 7, 3000, 1, 64, 20000, 3, 9000, 2050])
    layout = BucketLayout.from_manifest(man)
    states = [synth.gen_state(man, i, synth.MODE_ADVERSARIAL) for i in range(n)]
    bk = states_to_buckets(layout, states, DEV)
    plan = lib.Plan(layout.segs32, layout.f32_numel, layout.segs64, layout.i64_numel,
                    flags=lib.FA_PLAN_GAPS_ARE_PADDING | lib.FA_PLAN_TUNE_NO_BALANCE)
    assert plan.launch_form(n, weighted)[2] == 0
    w = O.weights_from_sizes(np.arange(1, n + 1) * 7 + 3) if weighted else None
    if w is None:
        want = O.aggregate_state(states)
    else:
        want = []
        for j, (k, v0) in enumerate(states[0]):
            x = np.stack([np.asarray(st[j][1]) for st in states])
            want.append((k, O.mean_i64_trunc(x) if x.dtype == np.int64 else O.weighted_sum0(x, w)))
    wa = None if w is None else (ctypes.c_float * n)(*[float(x) for x in w])
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fl in (0, lib.FA_F_BCAST):
        o32 = torch.full_like(bk[0][0], np.nan)
        o64 = torch.full_like(bk[0][1], -7)
        lib.check(lib.lib.fa_reduce(plan.handle, lib.ptr_array([b[0].data_ptr() for b in bk]),
                                    lib.ptr_array([b[1].data_ptr() for b in bk]), n, wa,
                                    o32.data_ptr(), o64.data_ptr(), fl, s))
        torch.cuda.synchronize()
        for (k, v), (_, g) in zip(want, buckets_to_state(layout, o32, o64)):
            assert bits_equal(g, v), (n, weighted, fl, k)
    for f, i in bk:   # the round's broadcast (the last call)
        for o, m in layout.segs32:
            assert torch.equal(f[o:o + m].view(torch.int32), o32[o:o + m].view(torch.int32)), o


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [2, 5, 7, 8, 11, 12, 16, 17, 20, 33, 63, 64, 100, 128, 200, 256, 300])
def test_client_loop_instances_on_a_long_launch(lib, n, weighted):
    """The client loop (reduce_impl.h pipe2_clients: the next client's loads
    before the current client's adds; the PIPE kernel instances) driven on
    purpose: a layout whose launch runs >= 3 rounds of resident
    workgroups (pipe_rule), default plan flags, and the choice asserted
    through fa_plan_launch_form — 2..7 and 12..63 clients take the loop on
    their full tiles (12..16 since r06), and unweighted 64..128 (r06) and
    from 256 over the device pointer table (pipe = 2, r06), the rest the
    batches.  Client data adversarial
    (2^-20 .. 2^20 magnitudes, generated on the device); the oracle checks
    every small tensor whole and windows of the long one — its head, middle
    and its end (the last partial tile and the ILP-4 tail columns), each
    window a whole-tensor oracle call over columns of the same class."""
    probe = lib.Plan(np.array([[0, 4096]], np.int64), 4096)
    slots = probe.launch_shape(n, weighted)[1]
    assert slots > 0
    big = 3 * slots * 2048 + 2050 + 13
    sizes = [100, 4096, 7, 3000, 1, 64, big, 3, 9000]
    man = {"keys": [{"key": f"k{j}", "shape": [m], "dtype": "float32"}
                    for j, m in enumerate(sizes)]}
    layout = BucketLayout.from_manifest(man)
    plan = lib.Plan(layout.segs32, layout.f32_numel, flags=lib.FA_PLAN_GAPS_ARE_PADDING)
    want_pipe = 1 if (2 <= n <= 7 or 12 <= n <= 63 or (not weighted and 64 <= n <= 128)) else 0
    if not weighted and n >= 256:
        want_pipe = 2          # the loop over the device pointer table (r06)
    assert plan.launch_form(n, weighted)[2] == want_pipe, (n, weighted, plan.launch_form(n, weighted))
    F = max(layout.f32_numel, 64)
    g = torch.Generator(device=DEV)
    g.manual_seed(1000 + n)
    x = torch.rand((n, F), generator=g, device=DEV) * 2 - 1
    ex = torch.randint(-20, 21, (n, F), generator=g, device=DEV).to(torch.float32)
    x = (x * torch.pow(2.0, ex)).contiguous()
    w = O.weights_from_sizes(np.arange(1, n + 1) * 7 + 3) if weighted else None
    wa = None if w is None else (ctypes.c_float * n)(*[float(v) for v in w])
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.full((F,), float("nan"), device=DEV)
    lib.check(lib.lib.fa_reduce(plan.handle, lib.ptr_array([x[i].data_ptr() for i in range(n)]),
                                None, n, wa, out.data_ptr(), None, 0, s))
    torch.cuda.synchronize()
    o_big, m_big = [(int(o), int(m)) for o, m in layout.segs32][6]
    t = m_big % 32
    windows = [(int(o), int(m)) for j, (o, m) in enumerate(layout.segs32) if j != 6]
    windows += [(o_big, 8192), (o_big + (m_big // 2) // 64 * 64, 8192),
                (o_big + m_big - 64 - t - 4096, 4096 + 64 + t)]
    for o, m in windows:
        cols = x[:, o:o + m].cpu().numpy()
        want = O.torch_mean0(cols) if w is None else O.weighted_sum0(cols, w)
        got = out[o:o + m].cpu().numpy()
        assert bits_equal(got, want), (n, weighted, o, m)


def test_round_one_plan_two_streams(lib):
    """A plan is read-only in a round: rounds on one plan issued on two
    streams without any host synchronisation are each exact (eight client
    sets of 5, the streams alternating)."""
    man = _rand_manifest(None, [4096, 33, 50000, 1, 7000])
    layout = BucketLayout.from_manifest(man)
    plan = lib.Plan(layout.segs32, layout.f32_numel, layout.segs64, layout.i64_numel,
                    flags=lib.FA_PLAN_GAPS_ARE_PADDING)
    sets, wants = [], []
    for k in range(8):
        states = [synth.gen_state(man, 10 * k + i, synth.MODE_ADVERSARIAL) for i in range(5)]
        sets.append(states_to_buckets(layout, states, DEV))
        wants.append(O.aggregate_state(states))
    outs = [(torch.full_like(b[0][0], np.nan), torch.full_like(b[0][1], -7)) for b in sets]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    for k, bk in enumerate(sets):
        st = streams[k % 2]
        lib.check(lib.lib.fa_reduce(plan.handle, lib.ptr_array([b[0].data_ptr() for b in bk]),
                                    lib.ptr_array([b[1].data_ptr() for b in bk]), 5, None,
                                    outs[k][0].data_ptr(), outs[k][1].data_ptr(), lib.FA_F_BCAST,
                                    ctypes.c_void_p(st.cuda_stream)))
    torch.cuda.synchronize()
    for k in range(8):
        for (key, v), (_, g) in zip(wants[k], buckets_to_state(layout, *outs[k])):
            assert bits_equal(g, v), (k, key)
        for f, i in sets[k]:
            for o, m in layout.segs32:
                assert torch.equal(f[o:o + m].view(torch.int32),
                                   outs[k][0][o:o + m].view(torch.int32))


def test_int64_adversarial(lib):
    man = {"keys": [{"key": f"i{j}", "shape": s, "dtype": "int64"}
                    for j, s in enumerate([[], [1], [3], [9], [40], [300]])]}
    layout = BucketLayout.from_manifest(man)
    for n in (1, 2, 7, 8, 9, 20, 33):
        states = [synth.gen_state(man, i, synth.MODE_ADVERSARIAL) for i in range(n)]
        out32, out64 = _reduce(lib, layout, states_to_buckets(layout, states, DEV))
        for (k, want), (_, g) in zip(O.aggregate_state(states),
                                     buckets_to_state(layout, out32, out64)):
            assert bits_equal(g, want), (n, k)


def test_synth_fill_matches_numpy(lib):
    stream = torch.cuda.current_stream().cuda_stream
    for mode in (0, 1):
        for key, name, shape in [(0, "a.weight", (64, 3, 3, 3)), (5, "b.running_var", (777,)),
                                 (9, "fc.weight", (10, 640))]:
            mu, sigma = synth.key_params(name, shape, "float32")
            numel = int(np.prod(shape))
            t = torch.empty(numel, dtype=torch.float32, device=DEV)
            lib.check(lib.lib.fa_synth_fill_f32(t.data_ptr(), numel, key, 3, mu, sigma, mode,
                                                ctypes.c_void_p(stream)))
            want = synth.gen_f32(key, numel, 3, mu, sigma, mode)
            assert bits_equal(t.cpu().numpy(), want), (mode, name)
        t = torch.empty(50, dtype=torch.int64, device=DEV)
        lib.check(lib.lib.fa_synth_fill_i64(t.data_ptr(), 50, 7, 2, mode, ctypes.c_void_p(stream)))
        assert np.array_equal(t.cpu().numpy(), synth.gen_i64(7, 50, 2, mode))


def test_stateless_abi(lib):
    n, M = 6, 3000
    x = np.random.default_rng(1).standard_normal((n, M)).astype(np.float32)
    segs = np.array([[0, 1000], [1024, 1976]], np.int64)
    bufs = [torch.from_numpy(np.concatenate([x[i, :1000], np.zeros(24, np.float32), x[i, 1000:2976]])).to(DEV)
            for i in range(n)]
    out = torch.zeros(3000, device=DEV)
    arr, ns = lib.seg_array(segs)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(lib.lib.fa_mean_f32(lib.ptr_array([b.data_ptr() for b in bufs]), n, 3000,
                                  out.data_ptr(), arr, ns, stream))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert bits_equal(o[:1000], O.torch_mean0(x[:, :1000]))
    assert bits_equal(o[1024:3000], O.torch_mean0(x[:, 1000:2976]))
    assert (o[1000:1024] == 0).all(), "stateless plan must not write gaps"
    w = O.weights_from_sizes([3, 1, 4, 1, 5, 9])
    lib.check(lib.lib.fa_weighted_f32(lib.ptr_array([b.data_ptr() for b in bufs]),
                                      (ctypes.c_float * n)(*map(float, w)), n, 3000,
                                      out.data_ptr(), arr, ns, stream))
    torch.cuda.synchronize()
    assert bits_equal(out.cpu().numpy()[:1000], O.weighted_sum0(x[:, :1000], w))
    iv = [torch.tensor([i * 1000003 - 5, 7 * i], dtype=torch.int64, device=DEV) for i in range(n)]
    o64 = torch.zeros(2, dtype=torch.int64, device=DEV)
    a64, n64 = lib.seg_array(np.array([[0, 1], [1, 1]], np.int64))
    lib.check(lib.lib.fa_mean_i64_trunc(lib.ptr_array([t.data_ptr() for t in iv]), n, 2,
                                        o64.data_ptr(), a64, n64, stream))
    torch.cuda.synchronize()
    xs = np.stack([t.cpu().numpy() for t in iv])
    assert o64.cpu().tolist() == [int(O.mean_i64_trunc(xs[:, 0])), int(O.mean_i64_trunc(xs[:, 1]))]


def test_errors(lib):
    from feddct_amd._lib import FedaggError
    layout = BucketLayout.from_manifest(_rand_manifest(None, [100]))
    with pytest.raises(FedaggError, match="FA_MAX_CLIENTS|exceeds"):
        bk = states_to_buckets(layout, [synth.gen_state({"keys": [
            {"key": "k0", "shape": [100], "dtype": "float32"},
            {"key": "nbt", "shape": [], "dtype": "int64"}]}, 0)], DEV)
        _reduce(lib, layout, bk * (lib.FA_MAX_CLIENTS + 1))
    misaligned = torch.zeros(200, device=DEV)[1:]
    plan = lib.Plan(layout.segs32, layout.f32_numel, layout.segs64, layout.i64_numel)
    rc = lib.lib.fa_reduce(plan.handle, lib.ptr_array([misaligned.data_ptr()]),
                           lib.ptr_array([misaligned.data_ptr()]), 1, None,
                           misaligned.data_ptr(), misaligned.data_ptr(), 0, None)
    assert rc == lib.FA_E_ALIGN


# ----------------------------------------------------------- drop-in shim --
def _modules(man, states):
    return [StateModule(man).load_numpy(s).to(DEV) for s in states]


@pytest.mark.parametrize("variant", ["fedavg", "fedprox"])
@pytest.mark.parametrize("mode", [synth.MODE_REALISTIC, synth.MODE_ADVERSARIAL])
def test_shim_matches_reference_goldens(golden, variant, mode):
    import importlib
    sa = importlib.import_module(f"feddct_amd.{variant}").server_aggregate
    man = golden["manifest"]["small"]
    gold = golden["gold"]
    for n in golden["manifest"]["ns"]:
        states = [synth.gen_state(man, i, mode) for i in range(n)]
        g = StateModule(man).to(DEV)
        clients = _modules(man, states)
        sa(g, clients)
        torch.cuda.synchronize()
        gsd = g.state_dict()
        for e in man["keys"]:
            k = e["key"]
            ref = gold[f"{variant}/m{mode}/n{n}/{k}"]
            assert bits_equal(gsd[k].cpu().numpy(), ref), (variant, n, k)
            for c in clients:
                assert bits_equal(c.state_dict()[k].cpu().numpy(), ref), "broadcast"


@pytest.mark.parametrize("variant", ["feddct", "splitfed"])
def test_shim_split_matches_reference_goldens(golden, variant):
    import importlib
    sa = importlib.import_module(f"feddct_amd.{variant}").server_aggregate
    mm, pm = golden["manifest"]["main"], golden["manifest"]["proxy"]
    gold = golden["gold"]
    for n in (5, 24):
        ms = _modules(mm, [synth.gen_state(mm, i, synth.MODE_ADVERSARIAL) for i in range(n)])
        ps = _modules(pm, [synth.gen_state(pm, 100 + i, synth.MODE_ADVERSARIAL) for i in range(n)])
        gm, gp = StateModule(mm).to(DEV), StateModule(pm).to(DEV)
        sa(gm, gp, ms, ps)
        torch.cuda.synchronize()
        for part, g, cl in (("main", gm, ms), ("proxy", gp, ps)):
            for k, v in g.state_dict().items():
                ref = gold[f"{variant}/n{n}/{part}/{k}"]
                assert bits_equal(v.cpu().numpy(), ref), (part, k)
                assert bits_equal(cl[-1].state_dict()[k].cpu().numpy(), ref)


def test_shim_host_resident_modules(golden):
    """The reference's CPU configuration (BASELINE config 1): modules in host
    memory, staged through the GPU and written back."""
    from feddct_amd.fedavg import server_aggregate
    man = golden["manifest"]["small"]
    gold = golden["gold"]
    n = 20
    states = [synth.gen_state(man, i, synth.MODE_ADVERSARIAL) for i in range(n)]
    g = StateModule(man)
    clients = [StateModule(man).load_numpy(s) for s in states]
    server_aggregate(g, clients)
    for k, v in g.state_dict().items():
        assert v.device.type == "cpu"
        assert bits_equal(v.numpy(), gold[f"fedavg/m1/n{n}/{k}"]), k
        assert bits_equal(clients[7].state_dict()[k].numpy(), gold[f"fedavg/m1/n{n}/{k}"])


def test_shim_second_round_and_rebind():
    """Arena binding persists across rounds; training-style in-place updates
    are seen; replacing a parameter triggers a re-bind."""
    from feddct_amd.fedavg import server_aggregate
    man = {"keys": [{"key": "w", "shape": [1000], "dtype": "float32"},
                    {"key": "n", "shape": [], "dtype": "int64"}]}
    states = [synth.gen_state(man, i, synth.MODE_ADVERSARIAL) for i in range(4)]
    g = StateModule(man).to(DEV)
    clients = _modules(man, states)
    server_aggregate(g, clients)
    with torch.no_grad():
        for i, c in enumerate(clients):
            c.w.mul_(float(i + 1))
            c.n.add_(i)
    clients[2].w = torch.nn.Parameter(clients[2].w.detach().clone() + 1)  # new object
    snap = [[(k, v.detach().cpu().numpy().copy()) for k, v in c.state_dict().items()]
            for c in clients]
    server_aggregate(g, clients)
    torch.cuda.synchronize()
    for (k, want) in O.aggregate_state(snap):
        assert bits_equal(g.state_dict()[k].cpu().numpy(), want), k
        assert bits_equal(clients[2].state_dict()[k].cpu().numpy(), want), k


@pytest.mark.parametrize("change", ["none", "inplace", "data_swap", "new_param", "dict_store",
                                    "new_buffer", "other_clients", "weighted",
                                    "global_data_swap", "global_new_param",
                                    "client_shape_swap", "client_shape_param",
                                    "client_same_bucket_review"])
@pytest.mark.parametrize("precheck", ["every_tensor", "use_counts"])
def test_bound_round_fast_path_sees_every_change(change, precheck, monkeypatch):
    """r04: a repeat server_aggregate on the same modules takes the bound
    round (Engine.try_bound_round); anything that changes what is bound must
    send it down the full path (re-bind), and every round equals the
    reference's arithmetic on the modules' values at call time.  r05
    (VERDICT r04 weak 6): a change on the GLOBAL model is caught before the
    reduce is launched — a tensor the caller kept on the global's old
    storage is left untouched, as the reference leaves it.  r06 (VERDICT r05
    next 2): so is a change on a client — one whose parameter was replaced by
    one of another shape (`.data` swap or a new Parameter) makes the call
    raise the reference's RuntimeError with the global and every client
    unchanged.  Both pre-launch checks run: every tensor (rounds of up to
    aggregate.BOUND_PRECHECK_MAX client tensors) and the bucket use counts
    (larger rounds, forced here with a limit of 0).  Pinned: under the use
    counts, a client tensor re-viewed onto ANOTHER part of its own bucket
    with another shape (the one change that leaves the counts alone) is seen
    only after the reduce — the call raises as the reference does, but the
    global then holds the reduce's result (shim.cpp bound_round)."""
    import gc
    import sys
    if sys.version_info >= (3, 12):
        pytest.skip("the fast path needs PEP 509 dict tags (CPython < 3.12)")
    from feddct_amd import aggregate as A
    from feddct_amd.fedavg import server_aggregate
    monkeypatch.setattr(A, "BOUND_PRECHECK_MAX", 4096 if precheck == "every_tensor" else 0)
    man = {"keys": [{"key": "w", "shape": [1000], "dtype": "float32"},
                    {"key": "b", "shape": [7], "dtype": "float32"},
                    {"key": "n", "shape": [], "dtype": "int64"}]}
    states = [synth.gen_state(man, i, synth.MODE_ADVERSARIAL) for i in range(5)]
    g = StateModule(man).to(DEV)
    clients = _modules(man, states)
    server_aggregate(g, clients)
    e = A.engine()
    assert e._round is not None
    assert e._round.native is not None   # the one-call C++ form (shim bound_round)
    calls = []
    orig = e.try_bound_round

    def spy(*a, **k):
        r = orig(*a, **k)
        calls.append(r)
        return r
    e.try_bound_round = spy
    try:
        with torch.no_grad():
            for i, c in enumerate(clients):
                c.w.mul_(float(i + 2))
        want_fast = change in ("none", "inplace")
        if change == "data_swap":
            clients[1].w.data = clients[1].w.data.clone() + 1
        elif change == "new_param":
            clients[3].b = torch.nn.Parameter(clients[3].b.detach().clone() - 2)
        elif change == "dict_store":
            clients[0]._parameters["b"] = torch.nn.Parameter(clients[0].b.detach().clone() * 3)
        elif change == "new_buffer":
            clients[2].register_buffer("extra_nonpersistent", torch.zeros(2, device=DEV),
                                       persistent=False)
        elif change == "other_clients":
            clients = clients[:4]
        if change in ("client_shape_swap", "client_shape_param", "client_same_bucket_review"):
            # r06: the reference raises inside
            # torch.stack and leaves every model untouched
            before = [{k: v.detach().cpu().numpy().tobytes() for k, v in m.state_dict().items()}
                      for m in [g] + clients]
            if change == "client_shape_swap":
                clients[1].w.data = torch.zeros(999, device=DEV)
            elif change == "client_shape_param":
                clients[3].b = torch.nn.Parameter(torch.zeros(8, device=DEV))
            else:   # w onto the bucket's b (7 floats of the same storage)
                clients[1].w.data = clients[1].b.data
            with pytest.raises(RuntimeError, match="stack expects each tensor to be equal size"):
                server_aggregate(g, clients)
            torch.cuda.synchronize()
            assert calls == [False], calls
            if change == "client_same_bucket_review" and precheck == "use_counts":
                return     # pinned above: the global holds the reduce's result
            for j, m in enumerate([g] + clients):
                for k, v in m.state_dict().items():
                    if (j, k) in ((2, "w"), (4, "b")):
                        continue   # the replaced tensor itself
                    assert v.detach().cpu().numpy().tobytes() == before[j][k], (change, j, k)
            return
        kept = None
        if change == "global_data_swap":
            kept = g.w.data                      # a view of the global's bound bucket
            g.w.data = g.w.data.clone() + 5
            want_fast = False
        elif change == "global_new_param":
            kept = g.b                           # the old parameter, on the bound bucket
            g.b = torch.nn.Parameter(g.b.detach().clone() - 2)
            want_fast = False
        kept_bytes = None if kept is None else kept.detach().cpu().numpy().tobytes()
        weights = None
        if change == "weighted":
            weights = [1.0, 2.0, 3.0, 4.0, 5.0]
        snap = [[(k, v.detach().cpu().numpy().copy()) for k, v in c.state_dict().items()]
                for c in clients]
        if weights is None:
            server_aggregate(g, clients)
        else:
            A.aggregate_weighted(g, clients, sizes=weights)
        torch.cuda.synchronize()
        assert calls and calls[0] == want_fast, (change, calls)
        if kept is not None:
            assert kept.detach().cpu().numpy().tobytes() == kept_bytes, change
        if weights is None:
            for (k, want) in O.aggregate_state(snap):
                assert bits_equal(g.state_dict()[k].cpu().numpy(), want), (change, k)
                for c in clients:
                    assert bits_equal(c.state_dict()[k].cpu().numpy(), want), (change, k)
        # and the round after the change is bound again
        calls.clear()
        snap = [[(k, v.detach().cpu().numpy().copy()) for k, v in c.state_dict().items()]
                for c in clients]
        server_aggregate(g, clients) if weights is None else A.aggregate_weighted(
            g, clients, sizes=weights)
        assert calls == [True]
        torch.cuda.synchronize()
        if weights is not None:
            # the bound weighted round equals the full path on fresh modules
            fresh = _modules(man, snap)
            g2 = StateModule(man).to(DEV)
            A.aggregate_weighted(g2, fresh, sizes=weights)
            torch.cuda.synchronize()
            for k, v in g2.state_dict().items():
                assert bits_equal(g.state_dict()[k].cpu().numpy(), v.cpu().numpy()), k
                for c in clients:
                    assert bits_equal(c.state_dict()[k].cpu().numpy(), v.cpu().numpy()), k
            del fresh, g2
    finally:
        del e.try_bound_round
    # the binding does not keep a dropped round alive
    del g, clients, snap
    gc.collect()
    assert e._round is None


@pytest.mark.parametrize("change", ["none", "inplace", "swap_order", "other_object",
                                    "new_param"])
def test_split_bound_round_fast_path(change):
    """r04: a repeat FedDCT / SplitFed call (server_aggregate_split) on the
    very objects of the last joint round takes the bound round without its
    pair lookups (_RoundBinding.split_ids, one identity check in C); any other
    objects, order or registration take the full path, and every round equals
    the reference's arithmetic on both halves."""
    import sys
    if sys.version_info >= (3, 12):
        pytest.skip("the fast path needs PEP 509 dict tags (CPython < 3.12)")
    from feddct_amd import aggregate as A
    from feddct_amd.feddct import server_aggregate
    mm = {"keys": [{"key": "w", "shape": [1000], "dtype": "float32"},
                   {"key": "b", "shape": [7], "dtype": "float32"},
                   {"key": "n", "shape": [], "dtype": "int64"}]}
    pm = {"keys": [{"key": "v", "shape": [300], "dtype": "float32"},
                   {"key": "m", "shape": [], "dtype": "int64"}]}
    n = 5
    ms = _modules(mm, [synth.gen_state(mm, i, synth.MODE_ADVERSARIAL) for i in range(n)])
    ps = _modules(pm, [synth.gen_state(pm, 100 + i, synth.MODE_ADVERSARIAL) for i in range(n)])
    gm, gp = StateModule(mm).to(DEV), StateModule(pm).to(DEV)
    server_aggregate(gm, gp, ms, ps)
    e = A.engine()
    assert e._round is not None and e._round.split_ids is not None
    calls = []
    orig = e._run_bound

    def spy(*a, **k):
        r = orig(*a, **k)
        calls.append(r)
        return r
    e._run_bound = spy
    try:
        with torch.no_grad():
            for i, c in enumerate(ms):
                c.w.mul_(float(i + 2))
        if change == "swap_order":
            ms, ps = [ms[1], ms[0]] + ms[2:], [ps[1], ps[0]] + ps[2:]
        elif change == "other_object":
            ms = ms[:4] + _modules(mm, [synth.gen_state(mm, 50, synth.MODE_ADVERSARIAL)])
        elif change == "new_param":
            ms[3].b = torch.nn.Parameter(ms[3].b.detach().clone() - 2)
        snaps = [[[(k, v.detach().cpu().numpy().copy()) for k, v in c.state_dict().items()]
                  for c in cl] for cl in (ms, ps)]
        server_aggregate(gm, gp, ms, ps)
        torch.cuda.synchronize()
        assert (bool(calls) and calls[0]) == (change in ("none", "inplace")), (change, calls)
        for g, cl, snap in ((gm, ms, snaps[0]), (gp, ps, snaps[1])):
            for k, want in O.aggregate_state(snap):
                assert bits_equal(g.state_dict()[k].cpu().numpy(), want), (change, k)
                for c in cl:
                    assert bits_equal(c.state_dict()[k].cpu().numpy(), want), (change, k)
        calls.clear()
        server_aggregate(gm, gp, ms, ps)
        assert calls == [True]
    finally:
        del e._run_bound


def test_shim_errors_like_reference():
    from feddct_amd.fedavg import server_aggregate
    man = {"keys": [{"key": "w", "shape": [10], "dtype": "float32"}]}
    g = StateModule(man).to(DEV)
    with pytest.raises(RuntimeError):
        server_aggregate(g, [])
    other = StateModule({"keys": [{"key": "v", "shape": [10], "dtype": "float32"}]}).to(DEV)
    with pytest.raises(KeyError):
        server_aggregate(g, [StateModule(man).to(DEV), other])
    bad = StateModule({"keys": [{"key": "w", "shape": [11], "dtype": "float32"}]}).to(DEV)
    with pytest.raises(RuntimeError):
        server_aggregate(g, [StateModule(man).to(DEV), bad])
    extra = StateModule({"keys": man["keys"] + [{"key": "z", "shape": [2], "dtype": "float32"}]})
    extra = extra.to(DEV)
    c0 = StateModule(man).to(DEV)
    with torch.no_grad():
        c0.w.fill_(2.0)
        extra.w.fill_(4.0)
    with pytest.raises(RuntimeError, match="Missing key"):
        server_aggregate(g, [c0, extra])
    assert torch.all(g.w == 3.0) and torch.all(c0.w == 3.0)  # global + earlier clients updated


def test_shim_mixed_dtypes_packed():
    """Non-fp32 floating keys and int32/bool buffers take the packed path
    (.float() -> mean -> copy_ back), as load_state_dict would."""
    from feddct_amd.fedavg import server_aggregate
    man = {"keys": [{"key": "h", "shape": [70], "dtype": "float16"},
                    {"key": "d", "shape": [33], "dtype": "float64"},
                    {"key": "b", "shape": [5], "dtype": "bool"},
                    {"key": "i", "shape": [4], "dtype": "int32"},
                    {"key": "f", "shape": [40], "dtype": "float32"}]}
    rng = np.random.default_rng(0)
    n = 5
    cpu_mods = []
    for i in range(n):
        m = StateModule(man)
        with torch.no_grad():
            m.h.copy_(torch.from_numpy(rng.standard_normal(70).astype(np.float16)))
            m.d.copy_(torch.from_numpy(rng.standard_normal(33)))
            m.b.copy_(torch.from_numpy(rng.integers(0, 2, 5).astype(bool)))
            m.i.copy_(torch.from_numpy(rng.integers(-99, 99, 4).astype(np.int32)))
            m.f.copy_(torch.from_numpy(rng.standard_normal(40).astype(np.float32)))
        cpu_mods.append(m)
    want = {}
    for k in ("h", "d", "b", "i", "f"):
        ref = torch.stack([m.state_dict()[k].float() for m in cpu_mods], 0).mean(0)
        t = cpu_mods[0].state_dict()[k].clone()
        t.copy_(ref)
        want[k] = t
    g = StateModule(man).to(DEV)
    clients = [m.to(DEV) for m in cpu_mods]
    server_aggregate(g, clients)
    torch.cuda.synchronize()
    for k, v in want.items():
        assert torch.equal(g.state_dict()[k].cpu(), v), k
        assert torch.equal(clients[3].state_dict()[k].cpu(), v), k


# ------------------------------------------------------ full-size digests --
def _full_case(lib, lay_name, n, device=DEV):
    man = load_manifest(lay_name)
    layout = BucketLayout.from_manifest(man)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bk = []
    for i in range(n):
        f32 = torch.zeros(layout.f32_numel, dtype=torch.float32, device=device)
        i64 = torch.zeros(max(1, layout.i64_numel), dtype=torch.int64, device=device)
        for j, e in enumerate(man["keys"]):
            s = layout.by_key[e["key"]]
            if s.kind == "i64":
                lib.check(lib.lib.fa_synth_fill_i64(i64[s.offset:].data_ptr(), s.numel, j, i, 0,
                                                    stream))
            else:
                mu, sigma = synth.key_params(e["key"], tuple(e["shape"]), e["dtype"])
                lib.check(lib.lib.fa_synth_fill_f32(f32[s.offset:].data_ptr(), s.numel, j, i,
                                                    mu, sigma, 0, stream))
        bk.append((f32, i64))
    out32, out64 = _reduce(lib, layout, bk)
    return O.state_digest(buckets_to_state(layout, out32, out64))


@pytest.mark.parametrize("case", ["fedavg/wrn16_8_c10/n2", "fedavg/wrn16_8_c10/n20",
                                  "fedprox/wrn16_8_c100/n20",
                                  "feddct/wrnsl16_8_sf4_c10_main/n5",
                                  "feddct/wrnsl16_8_sf4_c10_proxy/n5",
                                  "feddct/wrnsl16_8_sf4_c100_main/n24",
                                  "feddct/wrnsl16_8_sf4_c100_proxy/n24"])
def test_full_size_digest_vs_reference(lib, golden, case):
    _, lay, nn = case.split("/")
    assert _full_case(lib, lay, int(nn[1:])) == golden["digests"][case]


# ------------------------------------------- partitions and host pipeline --
@pytest.mark.parametrize("parts", [1, 3, 8, 64])
def test_range_plans_union_is_bit_exact(lib, parts):
    from feddct_amd.partition import range_plans
    man = load_manifest("wrnsl16_8_sf4_c10_proxy")
    layout = BucketLayout.from_manifest(man)
    from feddct_amd.workload import make_clients
    n = 7
    cl = make_clients(layout, man, range(n), DEV, synth.MODE_ADVERSARIAL)
    full32, full64 = _reduce(lib, layout, cl)
    ranges, p64 = range_plans(layout, parts)
    out32 = torch.full_like(full32, np.nan)
    out64 = torch.full_like(full64, -1)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    a32 = lib.ptr_array([c[0].data_ptr() for c in cl])
    a64 = lib.ptr_array([c[1].data_ptr() for c in cl])
    for lo, hi, plan in ranges:
        if plan is not None:
            lib.check(lib.lib.fa_reduce(plan.handle, a32, a64, n, None, out32.data_ptr(),
                                        out64.data_ptr(), 0, stream))
    lib.check(lib.lib.fa_reduce(p64.handle, a32, a64, n, None, out32.data_ptr(),
                                out64.data_ptr(), 0, stream))
    torch.cuda.synchronize()
    for s in layout.slots:
        if s.kind == "i64":
            assert torch.equal(out64[s.offset:s.offset + s.numel], full64[s.offset:s.offset + s.numel])
        else:
            a = out32[s.offset:s.offset + s.numel].cpu().numpy()
            b = full32[s.offset:s.offset + s.numel].cpu().numpy()
            assert bits_equal(a, b), s.key


@pytest.mark.parametrize("nchunks,fanout", [(6, "dma"), (6, "host"), (0, "host"), (0, "dma")])
def test_host_pipeline_bit_exact_with_broadcast(lib, nchunks, fanout):
    from feddct_amd.pipeline import HostPipeline
    from feddct_amd.workload import make_clients
    man = load_manifest("wrn16_8_c10")
    layout = BucketLayout.from_manifest(man)
    n = 5
    cl = make_clients(layout, man, range(n), DEV)
    full32, full64 = _reduce(lib, layout, cl)
    h32 = [c[0].cpu().pin_memory() for c in cl]
    h64 = [c[1].cpu().pin_memory() for c in cl]
    o32 = torch.zeros_like(h32[0]).pin_memory()
    o64 = torch.zeros_like(h64[0]).pin_memory()
    pipe = HostPipeline(layout, n, DEV, nchunks=nchunks, fanout=fanout)
    want = buckets_to_state(layout, full32, full64)

    def same(b32, b64):
        return all(bits_equal(a, b) for (_, a), (_, b) in
                   zip(buckets_to_state(layout, b32, b64), want))

    def clear():   # a download that is skipped must not leave the last round's result
        o32.fill_(7.25)
        o64.fill_(-3)
    for _ in range(2):  # second round reuses the device buffers
        clear()
        pipe.run(h32, h64, o32, o64)
        assert same(o32, o64)
    clear()
    pipe.run(h32, h64, o32, o64, h32[1:3], h64[1:3])
    assert same(h32[2], h64[2]) and same(h32[1], h64[1]) and same(o32, o64)
    # the reference's broadcast: every client's own (input) bucket receives
    # the global while later chunks still upload from those same buckets
    for i in (1, 2):
        h32[i].copy_(cl[i][0].cpu())
        h64[i].copy_(cl[i][1].cpu())
    clear()
    pipe.run(h32, h64, o32, o64, h32, h64)
    assert same(o32, o64) and all(same(a, b) for a, b in zip(h32, h64))


# ------------------------------------------------ FedProx proximal term --
def _prox_models(seed, same=False):
    torch.manual_seed(seed)
    mk = lambda: torch.nn.Sequential(torch.nn.Conv2d(3, 16, 3), torch.nn.BatchNorm2d(16),  # noqa
                                     torch.nn.Conv2d(16, 33, 3, bias=False), torch.nn.Linear(7, 5)).to(DEV)
    c, g = mk(), mk()
    if same:
        g.load_state_dict(c.state_dict())
    return c, g


@pytest.mark.parametrize("same", [False, True])
def test_proximal_term_matches_reference_loop(same):
    from feddct_amd.prox import proximal_term
    c, g = _prox_models(0, same)
    c_ref, g_ref = _prox_models(0, same)
    # reference: train_fedprox.py:113-115 on plain modules
    pt = 0.0
    for w, w_t in zip(c_ref.parameters(), g_ref.parameters()):
        pt += (w - w_t).norm(2)
    (pt * 0.37).backward()
    got = proximal_term(c, g)
    (got * 0.37).backward()
    torch.cuda.synchronize()
    torch.testing.assert_close(got, pt.detach(), rtol=2e-6, atol=1e-7)
    for (n, p), p_ref in zip(c.named_parameters(), c_ref.parameters()):
        torch.testing.assert_close(p.grad, p_ref.grad, rtol=1e-5, atol=1e-8, msg=n)
    for p, p_ref in zip(g.parameters(), g_ref.parameters()):
        torch.testing.assert_close(p.grad, p_ref.grad, rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("set_to_none", [True, False])
def test_proximal_term_flat_grads_in_a_training_loop(set_to_none):
    """The one-node proximal term (r03, flat_grads=True) inside the
    reference's step (train_fedprox.py:112-127): task loss + mu/2 * term,
    gradients accumulated over two iterations before each optimizer step
    (iters_to_accumulate), zero_grad either way.  Gradients and parameters
    track the per-parameter autograd form step by step."""
    from feddct_amd.prox import proximal_term
    runs = {}
    for flat in (True, False):
        c, g = _prox_models(2)
        opt = torch.optim.SGD(c.parameters(), lr=0.05, momentum=0.9)
        gen = torch.Generator(device=DEV).manual_seed(3)
        hist = []
        for it in range(6):
            x = torch.randn(4, 7, device=DEV, generator=gen)
            loss = c[3](x).square().sum() + 0.005 * proximal_term(c, g, flat_grads=flat)
            loss.backward()
            if it % 2 == 1:
                hist.append([p.grad.clone() for p in c.parameters()]
                            + [p.grad.clone() for p in g.parameters()])
                opt.step()
                opt.zero_grad(set_to_none=set_to_none)
        runs[flat] = (hist, [p.detach().clone() for p in c.parameters()])
    for ga, gb in zip(runs[True][0], runs[False][0]):
        for a, b in zip(ga, gb):
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)
    for a, b in zip(runs[True][1], runs[False][1]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)


def test_proximal_term_one_node_is_the_cpp_node():
    """r04: flat_grads=True builds the C++ autograd node (shim.cpp ProxNode):
    its backward equals the Python one-node definition, twice in a row
    (accumulation), and a double backward raises."""
    from feddct_amd.prox import proximal_term
    c1, g1 = _prox_models(5)
    c2, g2 = _prox_models(5)
    t = proximal_term(c1, g1, flat_grads=True)
    assert t.grad_fn is not None and "FedAggProximalTerm" in t.grad_fn.name()
    for _ in range(2):
        (0.3 * proximal_term(c1, g1, flat_grads=True)).backward()
        term = c2.__dict__.setdefault("_fa_prox", {}).get(id(g2))
        if term is None:
            proximal_term(c2, g2)          # binds the term
            term = c2.__dict__["_fa_prox"][id(g2)]
        from feddct_amd.prox import _ProxFlat
        _, anchor, _ = term._flat_state()
        (0.3 * _ProxFlat.apply(term, anchor)).backward()
    torch.cuda.synchronize()
    for a, b in zip(list(c1.parameters()) + list(g1.parameters()),
                    list(c2.parameters()) + list(g2.parameters())):
        torch.testing.assert_close(a.grad, b.grad, rtol=0, atol=0)
    x = proximal_term(c1, g1, flat_grads=True)
    anchor = c1.__dict__["_fa_prox"][id(g1)]._flat_state()[1]
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(x, [anchor], create_graph=True)


def test_proximal_term_one_node_outlives_its_term():
    """the C++ node's state OWNS the norm plan and both
    arena buckets.  Forward, then drop the cached term (and, in the second
    case, the client module itself), gc.collect(), then backward: the
    gradients equal those of a twin that kept everything alive."""
    import gc

    from feddct_amd.prox import proximal_term
    twin_c, twin_g = _prox_models(7)
    (0.4 * proximal_term(twin_c, twin_g, flat_grads=True)).backward()
    torch.cuda.synchronize()
    want_c = [p.grad.clone() for p in twin_c.parameters()]
    want_g = [p.grad.clone() for p in twin_g.parameters()]
    # the term dropped from the client's cache before backward
    c1, g1 = _prox_models(7)
    t1 = proximal_term(c1, g1, flat_grads=True)
    c1.__dict__["_fa_prox"].clear()
    gc.collect()
    (0.4 * t1).backward()
    torch.cuda.synchronize()
    for a, b in zip(list(c1.parameters()) + list(g1.parameters()), want_c + want_g):
        torch.testing.assert_close(a.grad, b, rtol=0, atol=0)
    # the client module dropped before backward (its parameters live on in
    # the node, as autograd keeps a graph's inputs)
    c3, g3 = _prox_models(7)
    t3 = proximal_term(c3, g3, flat_grads=True)
    cparams = list(c3.parameters())
    del c3
    gc.collect()
    (0.4 * t3).backward()
    torch.cuda.synchronize()
    for a, b in zip(cparams + list(g3.parameters()), want_c + want_g):
        torch.testing.assert_close(a.grad, b, rtol=0, atol=0)
    del t1, t3, cparams
    gc.collect()
    torch.cuda.synchronize()


def test_proximal_term_default_works_with_autograd_grad():
    """the default form is an ordinary autograd node over the
    parameters, so torch.autograd.grad(loss, params) and
    backward(inputs=params) see the proximal gradient; the opt-in one-node
    form is pruned from them (documented: its node has no parameter inputs),
    which this test pins so the caveat cannot silently change."""
    from feddct_amd.prox import proximal_term
    c, g = _prox_models(4)
    c_ref, g_ref = _prox_models(4)
    x = torch.randn(4, 7, device=DEV)
    pt = sum((w - w_t).norm(2) for w, w_t in zip(c_ref.parameters(), g_ref.parameters()))
    want = torch.autograd.grad(c_ref[3](x).square().sum() + 0.5 * pt, list(c_ref.parameters()))
    got = torch.autograd.grad(c[3](x).square().sum() + 0.5 * proximal_term(c, g),
                              list(c.parameters()))
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)
    # backward(inputs=...) on the default form: the global side untouched
    loss = c[3](x).square().sum() + 0.5 * proximal_term(c, g)
    loss.backward(inputs=list(c.parameters()))
    for a, b in zip(c.parameters(), want):
        torch.testing.assert_close(a.grad, b, rtol=1e-5, atol=1e-7)
    assert all(p.grad is None for p in g.parameters())
    # the one-node form is pruned by autograd.grad: only the task gradient
    task = torch.autograd.grad(c_ref[3](x).square().sum(), list(c_ref.parameters()),
                               allow_unused=True)
    flat = torch.autograd.grad(c[3](x).square().sum() + 0.5 * proximal_term(c, g, flat_grads=True),
                               list(c.parameters()), allow_unused=True)
    for a, b in zip(flat, task):
        assert (a is None) == (b is None)
        if a is not None:
            torch.testing.assert_close(a, b)


def test_proximal_term_tracks_training_and_aggregation():
    """Across an optimizer step and a server round the bound term stays
    current (params are arena views)."""
    from feddct_amd.fedprox import server_aggregate
    from feddct_amd.prox import proximal_term
    c, g = _prox_models(1)
    opt = torch.optim.SGD(c.parameters(), lr=0.1)
    for _ in range(3):
        opt.zero_grad()
        loss = c[3](torch.randn(4, 7, device=DEV)).square().sum() + 0.5 * proximal_term(c, g)
        loss.backward()
        opt.step()
        ref = sum((w - w_t).norm(2) for w, w_t in zip(c.parameters(), g.parameters()))
        torch.testing.assert_close(proximal_term(c, g).detach(), ref.detach(), rtol=2e-6, atol=1e-7)
    server_aggregate(g, [c])
    assert float(proximal_term(c, g)) == 0.0


def test_checkpoint_from_device_bucket(tmp_path):
    from feddct_amd.checkpoint import bucket_state_dict, load_into, save_checkpoint
    from feddct_amd.fedavg import server_aggregate
    man = load_manifest("wrnsl16_8_sf4_c10_main")
    states = [synth.gen_state(man, i) for i in range(3)]
    g = StateModule(man).to(DEV)
    cl = _modules(man, states)
    server_aggregate(g, cl)
    p = save_checkpoint({"round": 1, "state_dict": g}, False, str(tmp_path))
    ck = torch.load(p, weights_only=True)
    for k, v in g.state_dict().items():
        assert torch.equal(ck["state_dict"][k], v.cpu()), k
    fresh = StateModule(man).to(DEV)
    server_aggregate(fresh, [StateModule(man).to(DEV)])  # bind it
    load_into(fresh, ck["state_dict"])
    for k, v in g.state_dict().items():
        assert torch.equal(fresh.state_dict()[k], v), k
    assert list(bucket_state_dict(g)) == list(g.state_dict())


@pytest.mark.parametrize("flags", ["batch8", "batch16", "no_balance", "tile1024", "tile4096"])
def test_tuning_flags_keep_bits(lib, flags):
    from feddct_amd.workload import make_clients
    man = load_manifest("wrnsl16_8_sf4_c10_proxy")
    layout = BucketLayout.from_manifest(man)
    n = 19
    cl = make_clients(layout, man, range(n), DEV, synth.MODE_ADVERSARIAL)
    ref32, ref64 = _reduce(lib, layout, cl)
    # r05: the launch-shape choices that remain (every other tuning flag
    # was removed, test_abi.py::test_removed_tuning_flags_are_refused)
    extra, tile = {"batch8": (lib.FA_PLAN_TUNE_BATCH8, 1024),
                   "batch16": (lib.FA_PLAN_TUNE_BATCH16, 2048),
                   "no_balance": (lib.FA_PLAN_TUNE_NO_BALANCE, 2048),
                   "tile1024": (0, 1024), "tile4096": (0, 4096)}[flags]
    plan = lib.Plan(layout.segs32, layout.f32_numel, layout.segs64, layout.i64_numel,
                    tile, lib.FA_PLAN_GAPS_ARE_PADDING | extra)
    from feddct_amd.workload import Reducer
    o32 = torch.full_like(ref32, np.nan)
    o64 = torch.full_like(ref64, -1)
    Reducer(layout, cl, o32, o64, plan=plan)()
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(buckets_to_state(layout, o32, o64), buckets_to_state(layout, ref32, ref64)):
        assert bits_equal(a, b), (flags, k)


def test_split_joint_bucket_and_fallback_errors(golden):
    from feddct_amd.feddct import server_aggregate
    mm, pm = golden["manifest"]["main"], golden["manifest"]["proxy"]
    n = 5
    ms = _modules(mm, [synth.gen_state(mm, i, synth.MODE_ADVERSARIAL) for i in range(n)])
    ps = _modules(pm, [synth.gen_state(pm, 100 + i, synth.MODE_ADVERSARIAL) for i in range(n)])
    gm, gp = StateModule(mm).to(DEV), StateModule(pm).to(DEV)
    server_aggregate(gm, gp, ms, ps)
    # both halves of a slot live in one bucket: one launch per round
    pair = ms[2]._fa_pairs[id(ps[2])]
    buf = pair._fa_arena.f32
    for t in list(ms[2].parameters()) + list(ps[2].parameters()):
        assert buf.data_ptr() <= t.data_ptr() < buf.data_ptr() + buf.numel() * 4
    torch.cuda.synchronize()
    for k, v in gp.state_dict().items():
        assert bits_equal(v.cpu().numpy(), golden["gold"][f"feddct/n5/proxy/{k}"]), k
    # a main client missing a key: the reference's KeyError, unprefixed
    bad = StateModule({"keys": mm["keys"][1:]}).to(DEV)
    with pytest.raises(KeyError) as ei:
        server_aggregate(gm, gp, ms[:2] + [bad], ps[:3])
    assert ei.value.args[0] == mm["keys"][0]["key"]


@pytest.mark.parametrize("tag,n", [("c10", 5), ("c100", 24)])
def test_full_size_joint_feddct_digest(lib, golden, tag, n):
    """FedDCT slot = main + proxy in ONE bucket (aggregate._Pair layout): one
    launch reproduces both reference digests."""
    from feddct_amd.workload import joint_manifest, make_clients
    mm = load_manifest(f"wrnsl16_8_sf4_{tag}_main")
    pm = load_manifest(f"wrnsl16_8_sf4_{tag}_proxy")
    layout = BucketLayout.from_manifest(joint_manifest([mm, pm]))
    cl = make_clients(layout, [(mm, "0."), (pm, "1.")], range(n), DEV)
    out32, out64 = _reduce(lib, layout, cl)
    state = buckets_to_state(layout, out32, out64)
    for pf, lay in (("0.", "main"), ("1.", "proxy")):
        part = [(k[2:], v) for k, v in state if k.startswith(pf)]
        assert O.state_digest(part) == golden["digests"][f"feddct/wrnsl16_8_sf4_{tag}_{lay}/n{n}"]


def _max_ulp(a: np.ndarray, b: np.ndarray) -> int:
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int(np.abs(ia - ib).max())


def test_distance_to_torch_gpu_mean(lib, record_property):
    """The reference's original runs averaged CUDA tensors; torch-ROCm's GPU
    mean uses another summation order than torch's CPU mean (which the engine
    reproduces exactly).  Measured on the box for this seeded cfg2 state
    (profiles/r02_distance_to_torch_gpu_mean.txt): 46.1 % of
    elements bit-identical, max 13,107 ULP (at a near-cancelling element),
    max error 3.63 eps x mean|x_i|.  Inputs and both orders are deterministic,
    so the bounds below are tight pins, not tolerances; the opt-in
    FA_ORDER_TORCH_GPU plan must be 0 ULP."""
    from feddct_amd.workload import make_clients
    man = load_manifest("wrn16_8_c10")
    layout = BucketLayout.from_manifest(man)
    n = 20
    cl = make_clients(layout, man, range(n), DEV)
    out32, _ = _reduce(lib, layout, cl)
    worst_ulp, worst_rel, same, total = 0, 0.0, 0, 0
    for o, m in layout.segs32:
        x = torch.stack([c[0][o:o + m] for c in cl], 0)
        gpu = x.mean(0).cpu().numpy()
        ours = out32[o:o + m].cpu().numpy()
        worst_ulp = max(worst_ulp, _max_ulp(ours, gpu))
        # error in units of fp32 eps x mean|x_i| (the scale of an N-term sum)
        scale = x.abs().mean(0).cpu().numpy().astype(np.float64) * 2.0 ** -23
        rel = np.abs(ours.astype(np.float64) - gpu) / np.maximum(scale, 1e-45)
        worst_rel = max(worst_rel, float(rel.max()))
        same += int((ours.view(np.uint32) == gpu.view(np.uint32)).sum())
        total += m
    record_property("max_ulp_vs_torch_gpu_mean", worst_ulp)
    record_property("max_err_eps_of_mean_abs_vs_torch_gpu_mean", worst_rel)
    print(f"vs torch GPU mean: bit-identical {same}/{total}, max ULP {worst_ulp}, "
          f"max error {worst_rel:.2f} eps x mean|x|")
    assert worst_ulp <= 13107
    assert worst_rel <= 3.7
    # and the opt-in torch-GPU order IS torch's GPU mean: 0 ULP everywhere
    plan = lib.Plan(layout.segs32, layout.f32_numel, layout.segs64, layout.i64_numel,
                    order=lib.FA_ORDER_TORCH_GPU, n=n)
    g32 = torch.zeros_like(out32)
    g64 = torch.zeros_like(cl[0][1])
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(lib.lib.fa_reduce(plan.handle, lib.ptr_array([c[0].data_ptr() for c in cl]),
                                lib.ptr_array([c[1].data_ptr() for c in cl]), n, None,
                                g32.data_ptr(), g64.data_ptr(), 0, s))
    torch.cuda.synchronize()
    for o, m in layout.segs32:
        gpu = torch.stack([c[0][o:o + m] for c in cl], 0).mean(0)
        assert _max_ulp(g32[o:o + m].cpu().numpy(), gpu.cpu().numpy()) == 0


def test_shim_empty_and_unit_tensors():
    """Keys with no elements or one element (shape [0], [1,1], []) as the
    reference's stack().mean(0) handles them."""
    from feddct_amd.fedavg import server_aggregate
    man = {"keys": [{"key": "e", "shape": [0], "dtype": "float32"},
                    {"key": "u", "shape": [1, 1], "dtype": "float32"},
                    {"key": "s", "shape": [], "dtype": "float32"},
                    {"key": "w", "shape": [37], "dtype": "float32"},
                    {"key": "e64", "shape": [0], "dtype": "int64"}]}
    n = 9
    states = [synth.gen_state(man, i, synth.MODE_ADVERSARIAL) for i in range(n)]
    g = StateModule(man).to(DEV)
    clients = _modules(man, states)
    server_aggregate(g, clients)
    torch.cuda.synchronize()
    cpu = [StateModule(man).load_numpy(s) for s in states]
    for k, v in g.state_dict().items():
        ref = torch.stack([c.state_dict()[k].float() for c in cpu], 0).mean(0)
        want = cpu[0].state_dict()[k].clone()
        want.copy_(ref)
        assert v.shape == want.shape and torch.equal(v.cpu(), want), k


def test_unit_key_between_aligned_keys_n9():
    """a 1-element fp32 key between two aligned keys (a scalar
    nn.Parameter or PReLU weight) gets the inner order only, never also the
    cascade of a vector run planned across it; n=9 makes the two orders
    differ.  Through the shim against the reference's own expression."""
    from feddct_amd.fedavg import server_aggregate
    man = {"keys": [{"key": "w", "shape": [37], "dtype": "float32"},
                    {"key": "s", "shape": [], "dtype": "float32"},
                    {"key": "w2", "shape": [37], "dtype": "float32"},
                    {"key": "a", "shape": [64], "dtype": "float32"},
                    {"key": "p", "shape": [1], "dtype": "float32"},
                    {"key": "b", "shape": [128], "dtype": "float32"}]}
    n = 9
    states = [synth.gen_state(man, i, synth.MODE_ADVERSARIAL) for i in range(n)]
    for rep in range(3):   # tile scheduling varies between launches
        g = StateModule(man).to(DEV)
        clients = _modules(man, states)
        server_aggregate(g, clients)
        torch.cuda.synchronize()
        for (k, want), (k2, v) in zip(O.aggregate_state(states), g.state_dict().items()):
            assert k == k2 and bits_equal(v.cpu().numpy(), want), (rep, k)


@pytest.mark.parametrize("case", ["weighted/wrn16_8_c10/n20/sizes_1_20",
                                  "weighted/wrn16_8_c100/n20/cfg4_sizes"])
def test_full_size_weighted_digest(lib, case):
    """the client-size-weighted reduction at full size
    (BASELINE config 4: wrn16_8 C100 x 20, quantity-skewed sizes) against the
    committed digest of the build's weighted definition (C oracle,
    tests/golden/make_weighted_digests.py) — the reference itself has no
    weights, so this definition is the pin."""
    import json
    import os
    from conftest import ROOT
    from feddct_amd.workload import make_clients
    with open(os.path.join(ROOT, "tests", "golden", "weighted_digests.json")) as f:
        d = json.load(f)[case]
    lay = case.split("/")[1]
    man = load_manifest(lay)
    layout = BucketLayout.from_manifest(man)
    cl = make_clients(layout, man, range(20), DEV)
    out32, out64 = _reduce(lib, layout, cl, weights=np.asarray(d["weights"], np.float32))
    assert O.state_digest(buckets_to_state(layout, out32, out64)) == d["digest"]
