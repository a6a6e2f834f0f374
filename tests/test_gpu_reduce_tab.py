"""fa_reduce_tab with a table the caller owns (include/fedagg.h): above
FA_INLINE_CLIENTS clients the pointers and weights travel in a device table
[n fp32 ptrs][n int64 ptrs][n weights] that kernels write (400 words per
launch) into exactly fa_table_bytes(n) bytes of the caller's memory, with no
allocation and no host copy, so the call can be captured into a graph and
replayed.  Every plan kind that reads the table — the default order
(weighted, unweighted, the sum, both broadcasts), the torch-GPU order, the
16-bit and the mixed plans — against its independent reference and against
fa_reduce on the same inputs, bit for bit; the table between guard bands,
its contents against the layout restated here; guard bands around every
buffer a kernel writes; the table reused by a second call with no
synchronisation; graph replay; the refusals."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_gpu_h16_kernel as H
import test_gpu_mixed16_kernel as M16
from feddct_amd import _lib
from feddct_amd.layout import KIND_I64
from oracle import torch_gpu_order as G
from oracle import torch_order as T

pytestmark = pytest.mark.gpu

L = _lib.lib
GUARD = 64                       # elements on each side of every buffer
G32, G64 = 0xdeadbeef, -0x0123456789abcdef
TGUARD, GT = 64, 0xa5            # bytes on each side of the table, and their value
PAD = _lib.FA_PLAN_GAPS_ARE_PADDING
BCAST, SUM_ONLY, BCAST_ONLY = _lib.FA_F_BCAST, _lib.FA_F_SUM_ONLY, _lib.FA_F_BCAST_ONLY

LENS = [1, 5, 7, 33, 100, 2048 + 8, 4097]      # every tile kind
LENS_DEEP = [1, 5, 33, 1060]                   # the 4,097-client layout
SEGS64 = [(0, 1), (1, 5)]                      # int64 keys [] and [5]
N64 = 6
NS = [128, 129, 160, 161, 320, 321]            # 0 / 323 / 400 / 403 / 800 / 803 table words


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def layout(lens, variant):
    """-> (segs, f32_numel, plan flags).  "pad": every key on the next
    multiple of 4 and three trailing elements: the gaps are padding and the
    plan covers the bucket, so FA_F_BCAST copies it flat.  "gaps": flags 0,
    odd offsets and one real gap of 70 floats: the per-tile broadcast, and no
    gap element may be written."""
    segs, off = [], 0
    for j, m in enumerate(lens):
        off = (off + 3) // 4 * 4 if variant == "pad" else off + (0, 3, 70, 13)[j % 4]
        segs.append((off, m))
        off += m
    return segs, off + 3, (PAD if variant == "pad" else 0)


def inside_mask(segs, numel):
    m = np.zeros(numel, bool)
    for o, k in segs:
        m[o:o + k] = True
    return m


def place(cols, segs, numel):
    """Columns laid into the segments in order; everything else the guard."""
    out = np.full((cols.shape[0], numel), G32, np.uint32)
    c = 0
    for o, m in segs:
        out[:, o:o + m] = cols[:, c:c + m].view(np.uint32)
        c += m
    return out


def gather(v, segs):
    return np.concatenate([v[..., o:o + m] for o, m in segs], -1)


@functools.lru_cache(maxsize=None)
def inputs(n, lens, seed=0):
    """(fp32 columns [n, sum(lens)], int64 [n, N64], weights): shared by the
    tests of one client count, never modified."""
    rng = np.random.default_rng(100 * n + seed)
    tot = sum(lens)
    cols = np.ldexp(rng.standard_normal((n, tot), dtype=np.float32),
                    rng.integers(-10, 11, (n, tot), dtype=np.int32))   # magnitudes 2^-10 .. 2^10
    assert cols.dtype == np.float32
    x64 =rng.integers(-(1 << 40), 1 << 40, (n, N64)).astype(np.int64)
    w = T.weights_from_sizes(rng.integers(10, 1000, n))
    for a in (cols, x64, w):
        a.setflags(write=False)
    return cols, x64, w


def key_slices(lens):
    out, c = [], 0
    for m in lens:
        out.append((c, m))
        c += m
    return out


@functools.lru_cache(maxsize=None)
def reference(n, lens, what, seed=0):
    """The oracle, per key, on the columns of inputs(): "mean" and "i64"
    through aggregate_state, "wsum" weighted_sum0, "sum" torch_sum0."""
    cols, x64, w = inputs(n, lens, seed)
    ks = key_slices(lens)
    if what in ("mean", "i64"):
        states = [[(f"k{j}", cols[i, c:c + m]) for j, (c, m) in enumerate(ks)]
                  + [(f"i{j}", x64[i, o:o + m]) for j, (o, m) in enumerate(SEGS64)]
                  for i in range(n)]
        res = T.aggregate_state(states)
        f = np.concatenate([v for k, v in res if k[0] == "k"]).astype(np.float32)
        i = np.concatenate([v for k, v in res if k[0] == "i"])
        assert i.dtype == np.int64
        return f if what == "mean" else i
    if what == "wsum":
        return np.concatenate([T.weighted_sum0(cols[:, c:c + m], w) for c, m in ks])
    assert what == "sum"
    return np.concatenate([T.torch_sum0(cols[:, c:c + m]) for c, m in ks])


class Table:
    """Exactly fa_table_bytes(n) bytes between two guard bands inside a
    larger device buffer."""

    def __init__(self, n):
        self.bytes = int(L.fa_table_bytes(n))
        self.t = torch.full((2 * TGUARD + self.bytes,), GT, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 8 == 0
        self.addr = self.t.data_ptr() + TGUARD
        self.ptr = ctypes.c_void_p(self.addr) if self.bytes else None

    def body(self):
        return self.t.cpu().numpy()[TGUARD:TGUARD + self.bytes]

    def assert_guards(self, what):
        h = self.t.cpu().numpy()
        assert (h[:TGUARD] == GT).all() and (h[TGUARD + self.bytes:] == GT).all(), \
            (what, "wrote outside fa_table_bytes(n)")


def expected_table(p32, p64, w):
    """The header's layout: n fp32 pointers, n int64 pointers, n weights
    (zeros on an unweighted call), as bytes."""
    n = len(p32)
    wv = np.zeros(n, np.float32) if w is None else np.asarray(w, np.float32)
    return np.concatenate([np.asarray(p32, np.uint64).view(np.uint8),
                           np.asarray(p64, np.uint64).view(np.uint8), wv.view(np.uint8)])


class Bufs:
    """n fp32 client buckets, the fp32 result bucket and the int64 buckets on
    the device, each between two guard bands (the idiom of
    test_gpu_mixed16_kernel.Bufs)."""

    def __init__(self, bits, x64, numel):
        n = bits.shape[0]
        self.n, self.numel = n, numel
        self.row = (numel + 3) // 4 * 4 + 2 * GUARD
        self.row64 = N64 + 2 * GUARD
        self.h32 = np.full((n, self.row), G32, np.uint32)
        self.h32[:, GUARD:GUARD + numel] = bits
        self.h64 = np.full((n, self.row64), G64, np.int64)
        self.h64[:, GUARD:GUARD + N64] = x64
        self.c32 = torch.empty((n, self.row), dtype=torch.int32, device="cuda")
        self.c64 = torch.empty((n, self.row64), dtype=torch.int64, device="cuda")
        self.o32 = torch.empty(numel + 2 * GUARD, dtype=torch.int32, device="cuda")
        self.o64 = torch.empty(self.row64, dtype=torch.int64, device="cuda")
        self.p32 = [self.c32.data_ptr() + 4 * (self.row * i + GUARD) for i in range(n)]
        self.p64 = [self.c64.data_ptr() + 8 * (self.row64 * i + GUARD) for i in range(n)]
        self.out32 = self.o32.data_ptr() + 4 * GUARD
        self.out64 = self.o64.data_ptr() + 8 * GUARD
        self.load()

    def load(self, g32=None, g64=None):
        """(Re)fill every buffer in place: the clients' values, the result
        buckets with the guard value or the given global state."""
        self.c32.copy_(torch.from_numpy(self.h32.view(np.int32)))
        self.c64.copy_(torch.from_numpy(self.h64))
        o = np.full(self.numel + 2 * GUARD, G32, np.uint32)
        o64 = np.full(self.row64, G64, np.int64)
        if g32 is not None:
            o[GUARD:GUARD + self.numel] = g32
            o64[GUARD:GUARD + N64] = g64
        self.o32.copy_(torch.from_numpy(o.view(np.int32)))
        self.o64.copy_(torch.from_numpy(o64))

    def call(self, plan, flags=0, weights=None, table=None, tab=True, rows=None, out=None,
             sync=True):
        rows = range(self.n) if rows is None else rows
        a32 = _lib.ptr_array([self.p32[i] for i in rows])
        a64 = _lib.ptr_array([self.p64[i] for i in rows])
        n = len(rows)
        w = None if weights is None else (ctypes.c_float * n)(*[float(v) for v in weights])
        o32, o64 = (self.out32, self.out64) if out is None else out
        if tab:
            rc = L.fa_reduce_tab(plan.handle, a32, a64, n, w, table, o32, o64, flags, stream_ptr())
        else:
            rc = L.fa_reduce(plan.handle, a32, a64, n, w, o32, o64, flags, stream_ptr())
        if sync:
            torch.cuda.synchronize()
        return rc

    def snapshot(self):
        """Host copies of every buffer, guards included."""
        return SimpleNamespace(
            o32=self.o32.cpu().numpy().view(np.uint32), o64=self.o64.cpu().numpy(),
            c32=self.c32.cpu().numpy().view(np.uint32), c64=self.c64.cpu().numpy())

    def assert_guards(self, s, what):
        assert (s.o32[:GUARD] == G32).all() and (s.o32[GUARD + self.numel:] == G32).all(), \
            (what, "out32 guards")
        assert (s.o64[:GUARD] == G64).all() and (s.o64[GUARD + N64:] == G64).all(), \
            (what, "out64 guards")
        assert (s.c32[:, :GUARD] == G32).all() and (s.c32[:, GUARD + self.numel:] == G32).all(), \
            (what, "client fp32 guards")
        assert (s.c64[:, :GUARD] == G64).all() and (s.c64[:, GUARD + N64:] == G64).all(), \
            (what, "client int64 guards")

    def assert_clients_untouched(self, s, what):
        assert np.array_equal(s.c32, self.h32) and np.array_equal(s.c64, self.h64), \
            (what, "the call wrote a client bucket")


def body32(b, s):
    return s.o32[GUARD:GUARD + b.numel]


def body64(s):
    return s.o64[GUARD:GUARD + N64]


def assert_bits(got, want, what):
    """uint32 patterns against float32 values (the data is NaN-free)."""
    wb = np.ascontiguousarray(want, np.float32).view(np.uint32)
    assert not np.isnan(want).any()
    bad = np.nonzero(got != wb)[0]
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], wb[bad[:5]])


def tab_and_plain(b, plan, flags, w, what, g32=None, g64=None, has64=True):
    """The call through a caller-owned table, then fa_reduce on the same
    inputs: every buffer equal, byte for byte, guards included; the table's
    guards intact and its words the restated layout (a plan without int64
    keys does not read that bucket: NULL pointers).  Returns the table call's
    snapshot."""
    table = Table(b.n)
    snaps = []
    for tab in (True, False):
        b.load(g32, g64)
        rc = b.call(plan, flags, w, table.ptr, tab)
        assert rc == _lib.FA_OK, (what, tab, L.fa_last_error())
        snaps.append(b.snapshot())
        if tab:
            table.assert_guards(what)
            if table.bytes:
                want = expected_table(b.p32, b.p64 if has64 else [0] * b.n, w)
                assert np.array_equal(table.body()[:want.size], want), (what, "table words")
            else:
                assert table.ptr is None
    for k in ("o32", "o64", "c32", "c64"):
        assert np.array_equal(getattr(snaps[0], k), getattr(snaps[1], k)), \
            (what, k, "fa_reduce_tab differs from fa_reduce")
    b.assert_guards(snaps[0], what)
    return snaps[0]


def make(n, lens, variant, seed=0):
    segs, numel, flags = layout(lens, variant)
    cols, x64, w = inputs(n, tuple(lens), seed)
    b = Bufs(place(cols, segs, numel), x64, numel)
    plan = _lib.Plan(np.asarray(segs, np.int64), numel, SEGS64, N64, flags=flags)
    return SimpleNamespace(segs=segs, numel=numel, flags=flags, b=b, plan=plan, w=w,
                           inside=inside_mask(segs, numel), lens=tuple(lens), n=n, seed=seed)


def check_reduce(c, s, weighted, what, which=None):
    which = which or ("wsum" if weighted else "mean")
    out = body32(c.b, s)
    assert_bits(gather(out, c.segs), reference(c.n, c.lens, which, c.seed), what)
    if not c.flags:
        assert (out[~c.inside] == G32).all(), (what, "wrote a gap that is not padding")
    assert np.array_equal(body64(s), reference(c.n, c.lens, "i64", c.seed)), (what, "int64")


def check_broadcast(c, s, src32, src64, what):
    """Every client bucket holds the result: the whole bucket of a plan that
    covers it, the segments alone (gaps unwritten) otherwise."""
    cl = s.c32[:, GUARD:GUARD + c.numel]
    if c.flags:
        assert (cl == src32[None, :]).all(), (what, "flat broadcast")
    else:
        assert (cl[:, c.inside] == src32[None, c.inside]).all(), (what, "per-tile broadcast")
        assert np.array_equal(cl[:, ~c.inside], c.b.h32[:, GUARD:GUARD + c.numel][:, ~c.inside]), \
            (what, "the broadcast wrote a gap that is not padding")
    assert (s.c64[:, GUARD:GUARD + N64] == src64[None, :]).all(), (what, "int64 broadcast")


# ---------------------------------------------------------- default order ----
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", NS + [4097])
def test_default_order_through_a_caller_table(n, weighted):
    """n = 128: no table (NULL accepted).  129: the smallest, odd, so the
    int64 pointers and the weights start at odd word offsets.  160 / 161 and
    320 / 321: one against two and two against three fill launches.  4097 on
    the reduced layout: the DEEP cascade's levels through 27 fill launches.
    Weighted calls above 128 read tabw."""
    assert L.fa_table_bytes(n) == (0 if n <= 128 else (20 * n + 7) // 8 * 8)
    lens = LENS_DEEP if n > 4096 else LENS
    for variant in ("pad", "gaps") if n <= 4096 else ("pad",):
        c = make(n, lens, variant)
        what = (n, variant, weighted)
        s = tab_and_plain(c.b, c.plan, 0, c.w if weighted else None, what)
        check_reduce(c, s, weighted, what)
        c.b.assert_clients_untouched(s, what)


@pytest.mark.parametrize("n", [320, 321])
def test_pointer_table_client_loop(n):
    """The unweighted calls of 256 clients and more run their full 2048-float
    tiles through the client loop that reads the pointer table (pipe = 2) —
    once the launch is three rounds of resident workgroups long.  The small
    layout alone is a handful of tiles, so 32-float keys (one tile each,
    flags 0: tiles never span keys) pad the launch to that length; the
    2056- and 4097-element keys supply the full tiles.  launch_form pins the
    form, so this case cannot silently stop covering the loop."""
    segs, numel, _ = layout(LENS, "gaps")
    _, slots = _lib.Plan(np.asarray(segs, np.int64), numel, SEGS64, N64, flags=0).launch_shape(n)
    nfill = 3 * slots + 16
    assert 0 < slots <= 4096
    lens = tuple(LENS) + (32,) * nfill
    off = (numel + 3) // 4 * 4
    segs = segs + [(off + 36 * j, 32) for j in range(nfill)]
    numel = off + 36 * nfill
    cols, x64, _ = inputs(n, lens, 1)
    b = Bufs(place(cols, segs, numel), x64, numel)
    plan = _lib.Plan(np.asarray(segs, np.int64), numel, SEGS64, N64, flags=0)
    assert plan.launch_form(n)[0] == 2048 and plan.launch_form(n)[2] == 2, plan.launch_form(n)
    s = tab_and_plain(b, plan, 0, None, ("pipe2", n))
    out = body32(b, s)
    nl = sum(LENS)
    lead = np.concatenate([T.torch_mean0(cols[:, c:c + m]) for c, m in key_slices(LENS)])
    assert_bits(gather(out, segs[:len(LENS)]), lead, ("pipe2", n, "layout keys"))
    # the 32-float keys: M = 32 is all cascade body, as is every column of
    # the [n, nfill * 32] block reduced at once (M % 32 == 0): the same order
    # per column, one oracle call
    fill = T.torch_mean0(cols[:, nl:])
    assert_bits(gather(out, segs[len(LENS):]), fill, ("pipe2", n, "32-float keys"))
    assert (out[~inside_mask(segs, numel)] == G32).all(), "wrote a gap"
    want64 = np.concatenate([T.mean_i64_trunc(x64[:, o:o + m]) for o, m in SEGS64])
    assert np.array_equal(body64(s), want64)
    b.assert_clients_untouched(s, ("pipe2", n))


@pytest.mark.parametrize("variant", ["pad", "gaps"])
@pytest.mark.parametrize("n", [129, 321])
def test_sum_and_broadcast_flags_through_the_table(n, variant):
    c = make(n, LENS, variant)
    b = c.b
    # the ordered sum, no /N (int64 keys still take the mean)
    what = (n, variant, "sum only")
    s = tab_and_plain(b, c.plan, SUM_ONLY, None, what)
    check_reduce(c, s, False, what, "sum")
    b.assert_clients_untouched(s, what)
    # the reduce, then the broadcast's launch
    for weighted in (False, True):
        what = (n, variant, "bcast", weighted)
        s = tab_and_plain(b, c.plan, BCAST, c.w if weighted else None, what)
        check_reduce(c, s, weighted, what)
        check_broadcast(c, s, body32(b, s), body64(s), what)
    # the broadcast alone: the global state into every client
    rng = np.random.default_rng(n)
    g32 = rng.standard_normal(c.numel).astype(np.float32).view(np.uint32)
    g64 = rng.integers(-(1 << 50), 1 << 50, N64)
    what = (n, variant, "bcast only")
    s = tab_and_plain(b, c.plan, BCAST_ONLY, None, what, g32, g64)
    assert np.array_equal(body32(b, s), g32) and np.array_equal(body64(s), g64), \
        (what, "the broadcast wrote its source")
    check_broadcast(c, s, g32, g64, what)


# ------------------------------------------------------- torch-GPU order ----
@pytest.mark.parametrize("variant", ["pad", "gaps"])
@pytest.mark.parametrize("n", [129, 300])
def test_torch_gpu_order_through_the_table(n, variant):
    """No one-element key; the int64 bucket keeps its [5] key behind a
    one-element gap, which nothing may write.  The keys are those inside
    the restated configurations (fa_torch_gpu_config): all of them at
    n = 129; at n = 300 torch splits the rows of the 5- and 7-element keys
    128 ways, beyond the restated S <= 16, so they and the int64 [5] key
    have no torch-GPU-order plan to run."""
    lens = tuple(m for m in LENS[1:] if L.fa_torch_gpu_config(n, m, None))
    segs64 = [s for s in SEGS64[1:] if L.fa_torch_gpu_config(n, s[1], None)]
    assert {33, 100, 2048 + 8, 4097} <= set(lens), lens
    if n == 129:
        assert lens == tuple(LENS[1:]) and segs64
    for m in lens + tuple(m for _, m in segs64):
        assert G.supported(n, m), (n, m)
    segs, numel, flags = layout(lens, variant)
    cols, x64, _ = inputs(n, lens, 2)
    b = Bufs(place(cols, segs, numel), x64, numel)
    plan = _lib.Plan(np.asarray(segs, np.int64), numel, segs64, N64, flags=flags,
                     order=_lib.FA_ORDER_TORCH_GPU, n=n)
    what = ("torch-gpu", n, variant)
    s = tab_and_plain(b, plan, 0, None, what, has64=bool(segs64))
    out = body32(b, s)
    want = np.concatenate([G.gpu_mean0(cols[:, c:c + m]) for c, m in key_slices(lens)])
    assert_bits(gather(out, segs), want, what)
    if not flags:
        assert (out[~inside_mask(segs, numel)] == G32).all(), (what, "wrote a gap")
    for o, m in segs64:
        assert np.array_equal(body64(s)[o:o + m], G.gpu_mean_i64_trunc(x64[:, o:o + m])), what
    covered = inside_mask(segs64, N64)
    assert (body64(s)[~covered] == G64).all(), (what, "wrote the int64 gap")
    b.assert_clients_untouched(s, what)


# ------------------------------------------------ 16-bit and mixed plans ----
def fake_layout(segs, segs64):
    """What test_gpu_h16_kernel.expected reads of a BucketLayout."""
    slots = [SimpleNamespace(kind="h16", key=f"k{j}", offset=o, numel=m, shape=(m,))
             for j, (o, m) in enumerate(segs)]
    slots += [SimpleNamespace(kind=KIND_I64, key=f"i{j}", offset=o, numel=m, shape=(m,))
              for j, (o, m) in enumerate(segs64)]
    return SimpleNamespace(slots=slots)


def call16(b, plan, flags, w, table, tab, out):
    wa = None if w is None else (ctypes.c_float * b.n)(*[float(v) for v in w])
    if tab:
        rc = L.fa_reduce_tab(plan.handle, b.a16, b.a64, b.n, wa, table, out, b.p64, flags,
                             stream_ptr())
    else:
        rc = L.fa_reduce(plan.handle, b.a16, b.a64, b.n, wa, out, b.p64, flags, stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [129, 257])
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("dtype", sorted(M16.TDT))
def test_16_bit_and_mixed_plans_through_the_table(dtype, mixed, n, weighted):
    """The TAB instances of the 16-bit kernels and the narrowing broadcast:
    the reduce alone and FA_F_BCAST, each against the oracle and against
    fa_reduce."""
    segs, numel, flags = M16.seg_list("aligned", 0)
    tdt = M16.TDT[dtype]
    data = "cancel" if n == 257 and not weighted else "realistic"
    x16 = H.make_inputs(dtype, n, data, numel, 1000 * n + weighted)
    bits = M16.bits_of16(x16)
    x64t = H.make_i64(n, N64, n)
    x64 = x64t.numpy()
    w = T.weights_from_sizes(np.random.default_rng(n).integers(10, 1000, n)) if weighted else None
    want64 = np.concatenate([T.mean_i64_trunc(x64[:, o:o + m]) for o, m in M16.SEGS64])
    if mixed:
        plan = M16.mixed_plan(dtype, segs, numel, flags, M16.SEGS64, N64)
        want32 = M16.oracle(bits, dtype, segs, w)
    else:
        plan = M16.pure_plan(dtype, segs, numel, flags, M16.SEGS64, N64)
        exp = H.expected(fake_layout(segs, M16.SEGS64), tdt, x16, x64t, w)
        want16 = np.concatenate([M16.bits_of16(exp[f"k{j}"]) for j in range(len(segs))])
        assert not any(torch.isnan(exp[f"k{j}"]).any() for j in range(len(segs)))
    g16 = M16.G16
    for fl in (0, BCAST):
        res = []
        for tab in (True, False):
            what = (dtype, mixed, n, weighted, fl, tab)
            b = M16.Bufs(dtype, bits, x64, numel)
            table = Table(n)
            o16 = torch.from_numpy(np.full(b.row, g16, np.uint16).view(np.int16)).cuda()
            out = b.p32 if mixed else o16.data_ptr() + 2 * M16.GUARD
            assert call16(b, plan, fl, w, table.ptr, tab, out) == _lib.FA_OK, \
                (what, L.fa_last_error())
            table.assert_guards(what)
            b.assert_guards(what)
            h16 = o16.cpu().numpy().view(np.uint16)
            G_ = M16.GUARD
            assert (h16[:G_] == g16).all() and (h16[G_ + numel:] == g16).all(), (what, "out16")
            if tab:
                want = expected_table([b.a16[i] for i in range(n)], [b.a64[i] for i in range(n)], w)
                assert np.array_equal(table.body()[:want.size], want), (what, "table words")
            got64 = b.o64.cpu().numpy()[G_:G_ + N64]
            assert np.array_equal(got64, want64), what
            cb = b.client_bits()
            if mixed:
                o = b.out_bits()
                M16.assert_f32_bits(M16.gather(o, segs), want32, what)
                if fl:
                    M16.assert_narrowed(cb, o, dtype, what)
                res.append((o.copy(), cb.copy(), h16.copy()))
            else:
                o = h16[G_:G_ + numel]
                assert np.array_equal(M16.gather(o, segs), want16), what
                if fl:
                    assert (cb == o[None, :]).all(), (what, "flat broadcast of the 16-bit bucket")
                res.append((o.copy(), cb.copy(), b.out_bits().copy()))
            if fl:
                assert (b.c64.cpu().numpy()[:, G_:G_ + N64] == want64[None, :]).all(), what
            else:
                assert np.array_equal(cb, bits), (what, "the reduce wrote a client")
        for a, c in zip(*res):
            assert np.array_equal(a, c), (dtype, mixed, n, weighted, fl,
                                          "fa_reduce_tab differs from fa_reduce")


# ------------------------------------------------------------ table reuse ----
def test_one_table_two_calls_no_synchronisation():
    """n = 161, then n = 129 on other clients, back to back on one stream
    with one table: stream order alone keeps the second call's fill behind
    the first call's reduce, each call writes only its own words (the words
    past fa_table_bytes(129) keep the first call's values), both results are
    right."""
    c = make(161, LENS, "pad")
    b = c.b
    table = Table(161)
    rows2 = list(range(160, 31, -1))                   # 129 clients, another order
    assert len(rows2) == 129
    o2_32 = torch.from_numpy(np.full(c.numel + 2 * GUARD, G32, np.uint32).view(np.int32)).cuda()
    o2_64 = torch.full((N64 + 2 * GUARD,), G64, dtype=torch.int64, device="cuda")
    w2 = T.weights_from_sizes(np.arange(1, 130))
    rc1 = b.call(c.plan, 0, c.w, table.ptr, sync=False)
    rc2 = b.call(c.plan, 0, w2, table.ptr, rows=rows2, sync=False,
                 out=(o2_32.data_ptr() + 4 * GUARD, o2_64.data_ptr() + 8 * GUARD))
    torch.cuda.synchronize()
    assert rc1 == _lib.FA_OK and rc2 == _lib.FA_OK, L.fa_last_error()
    s = b.snapshot()
    check_reduce(c, s, True, "first call (161)")
    b.assert_guards(s, "reuse")
    b.assert_clients_untouched(s, "reuse")
    cols, x64, _ = inputs(161, tuple(LENS))
    h = o2_32.cpu().numpy().view(np.uint32)
    assert (h[:GUARD] == G32).all() and (h[GUARD + c.numel:] == G32).all()
    want = np.concatenate([T.weighted_sum0(cols[rows2, a:a + m], w2) for a, m in key_slices(LENS)])
    assert_bits(gather(h[GUARD:GUARD + c.numel], c.segs), want, "second call (129)")
    h64 = o2_64.cpu().numpy()
    assert (h64[:GUARD] == G64).all() and (h64[GUARD + N64:] == G64).all()
    want64 = np.concatenate([T.mean_i64_trunc(x64[rows2, o:o + m]) for o, m in SEGS64])
    assert np.array_equal(h64[GUARD:GUARD + N64], want64)
    table.assert_guards("reuse")
    t1 = expected_table(b.p32, b.p64, c.w)
    t2 = expected_table([b.p32[i] for i in rows2], [b.p64[i] for i in rows2], w2)
    body = table.body()
    assert np.array_equal(body[:t2.size], t2), "the second call's words"
    k = int(L.fa_table_bytes(129))
    assert np.array_equal(body[k:t1.size], t1[k:]), "the second call wrote past its own table"


# ----------------------------------------------------------- graph replay ----
@pytest.mark.parametrize("kind,n,weighted", [("f32", 129, False), ("f32", 129, True),
                                             ("f32", 321, False), ("f32", 321, True),
                                             ("mixed", 129, False)])
def test_captured_call_replays_from_the_table(kind, n, weighted):
    """One fa_reduce_tab call captured on a single stream (a linear chain:
    the fill launches, the reduce, the broadcast).  The arguments are frozen
    at capture: with the host pointer and weight arrays overwritten, the
    device table wiped and the client buckets rewritten in place, a replay
    gives the oracle's result for the new values under the captured weights,
    and the table holds the captured words again."""
    rng = np.random.default_rng(7 * n + weighted)
    w = T.weights_from_sizes(rng.integers(10, 1000, n)) if weighted else None
    if kind == "f32":
        segs, numel, pflags = layout(LENS, "pad")
        flags = 0
        tot = sum(LENS)

        def fresh():
            return (rng.standard_normal((n, tot)) * 10.0 ** rng.integers(-3, 4, (n, tot))
                    ).astype(np.float32)
        cols = fresh()
        b = Bufs(place(cols, segs, numel), rng.integers(-(1 << 40), 1 << 40, (n, N64)), numel)
        plan = _lib.Plan(np.asarray(segs, np.int64), numel, SEGS64, N64, flags=pflags)
        a32, a64 = _lib.ptr_array(b.p32), _lib.ptr_array(b.p64)
        p32, p64 = list(b.p32), list(b.p64)
        out32, out64 = b.out32, b.out64
    else:
        segs, numel, pflags = M16.seg_list("aligned", 0)
        flags = BCAST
        bits = M16.bits_of16(H.make_inputs("bfloat16", n, "realistic", numel, 1))
        b = M16.Bufs("bfloat16", bits, H.make_i64(n, N64, 1).numpy(), numel)
        plan = M16.mixed_plan("bfloat16", segs, numel, pflags, M16.SEGS64, N64)
        a32, a64 = b.a16, b.a64
        p32, p64 = [a32[i] for i in range(n)], [a64[i] for i in range(n)]
        out32, out64 = b.p32, b.p64
    wa = None if w is None else (ctypes.c_float * n)(*[float(v) for v in w])
    table = Table(n)
    want_table = expected_table(p32, p64, w)

    def call():
        return L.fa_reduce_tab(plan.handle, a32, a64, n, wa, table.ptr, out32, out64, flags,
                               stream_ptr())

    def check(cols_or_bits, x64, what):
        if kind == "f32":
            s = b.snapshot()
            got = gather(body32(b, s), segs)
            want = np.concatenate([T.torch_mean0(cols_or_bits[:, c:c + m]) if w is None
                                   else T.weighted_sum0(cols_or_bits[:, c:c + m], w)
                                   for c, m in key_slices(LENS)])
            assert_bits(got, want, what)
            got64 = body64(s)
            b.assert_guards(s, what)
        else:
            o = b.out_bits()
            M16.assert_f32_bits(M16.gather(o, segs), M16.oracle(cols_or_bits, "bfloat16", segs, w),
                                what)
            M16.assert_narrowed(b.client_bits(), o, "bfloat16", what)
            got64 = b.o64.cpu().numpy()[M16.GUARD:M16.GUARD + N64]
            b.assert_guards(what)
        want64 = np.concatenate([T.mean_i64_trunc(x64[:, o:o + m]) for o, m in SEGS64])
        assert np.array_equal(got64, want64), (what, "int64")
        table.assert_guards(what)
        assert np.array_equal(table.body()[:want_table.size], want_table), (what, "table words")

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                       # warm up on the capture stream
        assert call() == _lib.FA_OK, L.fa_last_error()
    side.synchronize()
    x64 = (b.h64 if kind == "f32" else b.c64.cpu().numpy())[:, GUARD:GUARD + N64].copy()
    if kind == "f32":
        check(cols, x64, "warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc = call()
    assert rc == _lib.FA_OK, L.fa_last_error()
    for i in range(n):                                  # frozen at capture: now garbage
        a32[i] = 0xdead0000 + 16 * i
        a64[i] = 0xbeef0000 + 8 * i
        if wa is not None:
            wa[i] = 1e30
    for rep in (1, 2):
        x64 = rng.integers(-(1 << 40), 1 << 40, (n, N64))
        if kind == "f32":
            new = fresh()
            b.h32[:, GUARD:GUARD + numel] = place(new, segs, numel)
            b.h64[:, GUARD:GUARD + N64] = x64
            b.load()                                    # in place: the same device buffers
        else:
            new = M16.bits_of16(H.make_inputs("bfloat16", n, "cancel", numel, 10 + rep))
            b.c16[:, GUARD:GUARD + numel] = torch.from_numpy(new.view(np.int16)).cuda()
            b.c64[:, GUARD:GUARD + N64] = torch.from_numpy(x64).cuda()
            b.o32[GUARD:GUARD + numel] = 0
            b.o64[GUARD:GUARD + N64] = 0
        table.t[TGUARD:TGUARD + table.bytes] = 0xff
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        check(new, x64, (kind, n, weighted, "replay", rep))


# --------------------------------------------------------------- refusals ----
def unchanged(b, table, before, tbefore, what):
    torch.cuda.synchronize()
    s = b.snapshot()
    for k in ("o32", "o64", "c32", "c64"):
        assert np.array_equal(getattr(s, k), getattr(before, k)), (what, k, "a refused call wrote")
    assert np.array_equal(table.t.cpu().numpy(), tbefore), (what, "a refused call wrote the table")


def test_refusals_launch_nothing():
    c = make(321, LENS, "pad")
    b = c.b
    table = Table(321)
    before, tbefore = b.snapshot(), table.t.cpu().numpy().copy()
    a32, a64 = _lib.ptr_array(b.p32), _lib.ptr_array(b.p64)

    def tab(plan, n, tptr, p32=a32):
        return L.fa_reduce_tab(plan.handle, p32, a64, n, None, tptr, b.out32, b.out64, 0,
                               stream_ptr())
    # a table that is not 8-B aligned
    for n in (129, 321):
        for d in (1, 4):
            assert tab(c.plan, n, ctypes.c_void_p(table.addr + d)) == _lib.FA_E_ALIGN
            assert b"8-B aligned" in L.fa_last_error()
            unchanged(b, table, before, tbefore, ("misaligned table", n, d))
    # ... matters only where a table is used
    assert tab(c.plan, 128, ctypes.c_void_p(table.addr + 4)) == _lib.FA_OK
    torch.cuda.synchronize()
    b.load()
    # a torch-GPU-order plan cut for another client count: refused before the fill
    lens = tuple(LENS[1:])
    segs, numel, flags = layout(lens, "pad")
    assert numel <= c.numel
    tg = _lib.Plan(np.asarray(segs, np.int64), numel, [SEGS64[1]], N64, flags=flags,
                   order=_lib.FA_ORDER_TORCH_GPU, n=129)
    assert tab(tg, 130, table.ptr) == _lib.FA_E_INVAL
    assert b"cut for n=129" in L.fa_last_error()
    unchanged(b, table, before, tbefore, "torch-GPU-order plan, other n")
    # a NULL client pointer far into the list
    holed = _lib.ptr_array(b.p32[:200] + [None] + b.p32[201:])
    assert tab(c.plan, 321, table.ptr, holed) == _lib.FA_E_INVAL
    assert b"client 200" in L.fa_last_error()
    unchanged(b, table, before, tbefore, "NULL client")
    # more clients than the library takes
    assert tab(c.plan, _lib.FA_MAX_CLIENTS + 1, table.ptr) == _lib.FA_E_RANGE
    unchanged(b, table, before, tbefore, "n > FA_MAX_CLIENTS")
    # and the table still works
    assert tab(c.plan, 321, table.ptr) == _lib.FA_OK
    torch.cuda.synchronize()
    check_reduce(c, b.snapshot(), False, "after the refusals")
