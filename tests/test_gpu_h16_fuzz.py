"""GPU fuzz of the 16-bit reduce (csrc/fedagg_h16.hip) on raw plans, the twin
of test_gpu_fuzz.py: segments at arbitrary element offsets (odd ones, keys
back to back, gaps that are or are not padding), bucket lengths of every
residue modulo 8, 1-257 clients, both tile widths, weighted and not, with and
without the broadcast — against the oracle bit for bit.  ``out`` and every
client bucket sit inside larger allocations with sentinel-filled guard bands:
nothing outside the bucket, and without FA_PLAN_GAPS_ARE_PADDING nothing
outside the segments, may change.

The case generator and the restated coverage rule need no GPU:
tests/test_h16_ref_cpu.py runs the same cases through the host planner, and
the last test here counts the case classes the seeds reach."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import torch_order as O

SEEDS = range(120)
SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 257, 1023, 2049, 4100]
NS = [1, 2, 3, 5, 8, 16, 17, 33, 127, 128, 129, 140, 257]
DTYPES = ("float16", "bfloat16")
TORCH_DT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
ELEM = {"float16": 1, "bfloat16": 2}          # FA_ELEM_F16, FA_ELEM_BF16
GAPS_ARE_PADDING, F_BCAST, F_BCAST_ONLY = 1, 1, 4   # include/fedagg.h
FLAT_PAD = 128        # a gap of this many 16-bit elements could hold a foreign key
GUARD = 136           # guard band (elements) in front of a bucket: >= 128, 16-B multiple
GUARD_PAT, OUT_PAT = 0x7e57, 0xabcd   # (a bf16 NaN and an fp16 value: nothing computes them)


def case(seed):
    """One raw case, from the seed alone."""
    rng = np.random.default_rng([seed, 16])
    dtype = DTYPES[seed % 2]
    mode = ("any", "any", "aligned8", "backtoback", "wide")[int(rng.integers(0, 5))]
    off = {"any": int(rng.integers(0, 20)), "aligned8": 8 * int(rng.integers(0, 4)),
           "backtoback": int(rng.integers(0, 9)), "wide": int(rng.integers(0, 140))}[mode]
    segs = []
    nseg = int(rng.integers(1, 10))
    for j in range(nseg):
        m = int(rng.choice(SIZES)) if rng.random() < 0.8 else int(rng.integers(1, 6000))
        if mode == "aligned8" and rng.random() < 0.5:
            # whole 32-column bodies: the vector run stays open behind such a
            # key, and only the padding flag lets the next key extend it
            m = int(rng.choice([32, 64, 96, 256, 2048, 4128]))
        if j == 0:
            m = max(m, 1)
        segs.append((off, m))
        gap = int(rng.integers(0, 71))
        if mode == "backtoback":
            gap = 0
        elif mode == "wide" and rng.random() < 0.4:
            gap = int(rng.integers(128, 200))
        elif mode == "aligned8":
            gap += -(off + m + gap) % 8
        off += m + gap
    end = segs[-1][0] + segs[-1][1]
    trail = int(rng.integers(0, 71)) if mode != "wide" else int(rng.integers(100, 200))
    numel = end + trail
    if numel % 2 != (seed // 2) % 2:     # half the buckets even, half odd
        numel += 1
    segs64, o64 = [], 0
    for _ in range(int(rng.integers(0, 4))):
        m = int(rng.choice([1, 1, 2, 5, 33, 100]))
        segs64.append((o64, m))
        o64 += m
    numel64 = o64 + (1 if o64 and rng.random() < 0.15 else 0)   # sometimes an unowned int64
    n = int(rng.choice(NS))
    return dict(seed=seed, dtype=dtype, mode=mode,
                segs=np.array(segs, np.int64).reshape(-1, 2), numel=numel,
                segs64=np.array(segs64, np.int64).reshape(-1, 2), numel64=numel64,
                n=n, tile=int(rng.choice([2048, 4096])), gaps_pad=bool(rng.random() < 0.55),
                weighted=bool(rng.random() < 0.36), bcast=bool(rng.random() < 0.5),
                naninf=bool(rng.random() < 0.1), rng=rng)


def gaps_of(segs, numel):
    """Lengths of the leading gap, the gaps between non-empty segments, and
    the trailing gap."""
    out, pos = [], 0
    for o, m in sorted((int(o), int(m)) for o, m in segs):
        if m == 0:
            continue
        out.append(o - pos)
        pos = o + m
    out.append(int(numel) - pos)
    return out


def flat_coverable(c):
    """The rule of include/fedagg.h (fa_plan_create_elem) and DESIGN §4.8,
    restated: a 16-bit plan may broadcast — a flat copy of the bucket's bytes
    as numel / 2 floats — only if the gaps are declared padding, the bucket
    has an even number of elements, no gap in front of, between or behind the
    floating segments has room for a key the plan does not own (128 elements
    or more), and the int64 segments leave no int64 element unowned."""
    return bool(c["gaps_pad"] and c["numel"] % 2 == 0
                and max(gaps_of(c["segs"], c["numel"])) < FLAT_PAD
                and max(gaps_of(c["segs64"], c["numel64"])) < 1)


def inside_mask(c):
    inside = np.zeros(c["numel"], bool)
    for o, m in c["segs"]:
        inside[o:o + m] = True
    return inside


def may_write_mask(c):
    """Elements of ``out`` the reduce may store to: the segments, and with
    the padding flag the gaps between two segments (never the bucket's head
    in front of the first segment or its tail behind the last)."""
    inside = inside_mask(c)
    if c["gaps_pad"] and inside.any():
        idx = np.nonzero(inside)[0]
        inside[idx[0]:idx[-1] + 1] = True
    return inside


# ----------------------------------------------------------------- inputs ----
def finite_patterns(rng, shape, dtype):
    """Random 16-bit patterns over the whole exponent range, subnormals and
    both zeros included, no inf / NaN."""
    b = rng.integers(0, 1 << 16, shape).astype(np.uint16)
    expo = np.uint16(0x7c00 if dtype == "float16" else 0x7f80)
    top = (b & expo) == expo
    b[top] &= np.uint16(~0x0400 & 0xffff if dtype == "float16" else ~0x0080 & 0xffff)
    return b


def make_clients(c):
    """bits[n, numel]: finite patterns in the segments (one client with a NaN
    and both infs in a tenth of the cases), arbitrary patterns — NaN included
    — in the gaps."""
    rng, n, numel, dtype = c["rng"], c["n"], c["numel"], c["dtype"]
    x = finite_patterns(rng, (n, numel), dtype)
    inside = inside_mask(c)
    if c["naninf"]:
        i = int(rng.integers(0, n))
        inf = 0x7c00 if dtype == "float16" else 0x7f80
        x[i, 0::7] = inf | 0x0201 if dtype == "float16" else inf | 0x0041   # a NaN
        x[i, 3::7] = inf
        x[i, 5::11] = inf | 0x8000
    raw = rng.integers(0, 1 << 16, (n, numel)).astype(np.uint16)
    raw[:, 0::3] = 0x7e01 if dtype == "float16" else 0x7fc1                  # NaN
    x[:, ~inside] = raw[:, ~inside]
    return x


def from_bits(bits, tdt):
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16).copy()).view(tdt)


def to_bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def expected_segments(c, x, weights):
    """Per non-empty floating segment: the oracle on the exactly widened
    values, then torch's CPU .to(dtype), as (bits, is-NaN)."""
    tdt = TORCH_DT[c["dtype"]]
    xf = from_bits(x, tdt).float().numpy()
    out = []
    for o, m in c["segs"]:
        if m == 0:
            out.append(None)
            continue
        with np.errstate(all="ignore"):
            r = O.torch_mean0(xf[:, o:o + m]) if weights is None \
                else O.weighted_sum0(xf[:, o:o + m], weights)
        t = torch.from_numpy(np.ascontiguousarray(r, np.float32)).to(tdt)
        out.append((to_bits(t), torch.isnan(t).numpy()))
    return out


class Arena:
    """``out`` and the client buckets inside larger allocations: GUARD
    sentinel elements in front of each bucket, at least 128 behind it, every
    bucket start 16-B aligned."""

    def __init__(self, c, x, x64, dev):
        n, numel = x.shape
        self.numel, self.n = numel, n
        self.row = (GUARD + numel + 128 + 7) // 8 * 8
        host = np.full((n + 1, self.row), GUARD_PAT, np.uint16)
        host[0, GUARD:GUARD + numel] = OUT_PAT
        host[1:, GUARD:GUARD + numel] = x
        self.host = host
        self.buf = torch.from_numpy(host.view(np.int16).copy()).to(dev)
        assert self.buf.data_ptr() % 16 == 0 and (2 * self.row) % 16 == 0 and (2 * GUARD) % 16 == 0
        self.n64 = max(1, c["numel64"])
        h64 = np.full((n + 1, self.n64 + 2), -3, np.int64)      # one guard word each side
        h64[1:, 1:1 + c["numel64"]] = x64
        self.host64 = h64
        self.buf64 = torch.from_numpy(h64.copy()).to(dev)
        base, base64 = self.buf.data_ptr(), self.buf64.data_ptr()
        self.out_ptr = base + 2 * GUARD
        self.client_ptrs = [base + 2 * ((i + 1) * self.row + GUARD) for i in range(n)]
        self.out64_ptr = base64 + 8
        self.client64_ptrs = [base64 + 8 * ((i + 1) * (self.n64 + 2) + 1) for i in range(n)]

    def read(self):
        """(out bits, client bits [n, numel], guards intact?, out64, clients64)"""
        g = self.buf.cpu().numpy().view(np.uint16)
        guards = np.ones(self.row, bool)
        guards[GUARD:GUARD + self.numel] = False
        ok = bool((g[:, guards] == GUARD_PAT).all())
        g64 = self.buf64.cpu().numpy()
        ok64 = bool((g64[:, 0] == -3).all() and (g64[:, -1] == -3).all())
        return (g[0, GUARD:GUARD + self.numel], g[1:, GUARD:GUARD + self.numel], ok and ok64,
                g64[0, 1:-1], g64[1:, 1:-1])


def launch(_lib, plan, ar, c, weights, flags):
    n = c["n"]
    has64 = len(c["segs64"]) > 0
    w = None if weights is None else (ctypes.c_float * n)(*[float(v) for v in weights])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib.fa_reduce(plan.handle, _lib.ptr_array(ar.client_ptrs),
                            _lib.ptr_array(ar.client64_ptrs) if has64 else None, n, w,
                            ar.out_ptr, ar.out64_ptr if has64 else None, flags, st)
    err = _lib.lib.fa_last_error() if rc else b""
    torch.cuda.synchronize()
    return rc, err


def setup(c):
    from feddct_amd import _lib
    assert (_lib.FA_PLAN_GAPS_ARE_PADDING, _lib.FA_F_BCAST, _lib.FA_F_BCAST_ONLY) == \
        (GAPS_ARE_PADDING, F_BCAST, F_BCAST_ONLY)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    plan = _lib.Plan(c["segs"], c["numel"], c["segs64"], c["numel64"], tile_elems=c["tile"],
                     flags=GAPS_ARE_PADDING if c["gaps_pad"] else 0, elem=ELEM[c["dtype"]])
    x = make_clients(c)
    x64 = c["rng"].integers(-2 ** 20, 2 ** 20, (c["n"], c["numel64"]), dtype=np.int64)
    return _lib, plan, x, x64, Arena(c, x, x64, dev)


def check_refused(_lib, rc, err, ar, what):
    assert rc == _lib.FA_E_INVAL and b"flat" in err, (what, rc, err)
    assert np.array_equal(ar.buf.cpu().numpy().view(np.uint16), ar.host), (what, "16-bit bytes")
    assert np.array_equal(ar.buf64.cpu().numpy(), ar.host64), (what, "int64 bytes")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_random_raw_plans_bit_exact(seed):
    c = case(seed)
    _lib, plan, x, x64, ar = setup(c)
    weights = O.weights_from_sizes(c["rng"].integers(1, 1000, c["n"])) if c["weighted"] else None
    flags = F_BCAST if c["bcast"] else 0
    coverable = flat_coverable(c)
    rc, err = launch(_lib, plan, ar, c, weights, flags)
    if c["bcast"] and not coverable:
        # refused before anything is launched; then the reduce alone
        check_refused(_lib, rc, err, ar, seed)
        rc, err = launch(_lib, plan, ar, c, weights, 0)
        flags = 0
    assert rc == 0, (seed, rc, err)      # (an accepted broadcast: the rule said coverable)
    out, clients, guards_ok, out64, clients64 = ar.read()
    assert guards_ok, (seed, "a guard band changed")
    for (o, m), want in zip(c["segs"], expected_segments(c, x, weights)):
        if want is None:
            continue
        wb, wn = want
        got = out[o:o + m]
        gn = torch.isnan(from_bits(got, TORCH_DT[c["dtype"]])).numpy()
        assert np.array_equal(gn, wn), (seed, o, m, "NaN positions")
        bad = np.nonzero((got != wb) & ~wn)[0]
        assert bad.size == 0, (seed, o, m, bad[:5], got[bad[:5]], wb[bad[:5]])
    for o, m in c["segs64"]:
        assert np.array_equal(out64[o:o + m], O.mean_i64_trunc(x64[:, o:o + m])), (seed, o, "int64")
    owned64 = np.zeros(ar.n64, bool)
    for o, m in c["segs64"]:
        owned64[o:o + m] = True
    assert (out64[~owned64] == -3).all(), (seed, "wrote an int64 element no segment owns")
    may = may_write_mask(c)
    assert (out[~may] == OUT_PAT).all(), (seed, "wrote outside the segments")
    if flags & F_BCAST:
        for i in range(c["n"]):
            assert np.array_equal(clients[i], out), (seed, i, "broadcast bytes", c["numel"] % 8)
            assert np.array_equal(clients64[i], out64), (seed, i, "broadcast int64")
    else:
        assert np.array_equal(clients, x), (seed, "a client bucket changed")
        assert np.array_equal(clients64[:, :c["numel64"]], x64), (seed, "a client int64 changed")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(0, 120, 8))
def test_broadcast_only_on_raw_plans(seed):
    """FA_F_BCAST_ONLY: out -> every client on a coverable plan, refused
    with nothing changed on every other."""
    c = case(seed)
    _lib, plan, x, x64, ar = setup(c)
    rc, err = launch(_lib, plan, ar, c, None, F_BCAST_ONLY)
    if not flat_coverable(c):
        check_refused(_lib, rc, err, ar, seed)
        return
    assert rc == 0, (seed, rc, err)
    out, clients, guards_ok, out64, clients64 = ar.read()
    assert guards_ok, (seed, "a guard band changed")
    assert (out == OUT_PAT).all() and (out64 == -3).all(), (seed, "the source changed")
    for i in range(c["n"]):
        assert np.array_equal(clients[i], out), (seed, i)
        if len(c["segs64"]):
            assert np.array_equal(clients64[i], out64), (seed, i)


def test_the_seeds_reach_every_case_class():
    """From the generator alone (no GPU): each class the 16-bit family was
    never given before is reached by at least 5 of the seeds."""
    count = dict.fromkeys(["odd offset", "offset not a multiple of 8", "back to back",
                           "non-padding gap", "odd numel", "refused broadcast",
                           "accepted broadcast with remainder", "weighted at N >= 129",
                           "weighted at N = 128", "gap >= 128", "naninf"], 0)
    for seed in SEEDS:
        c = case(seed)
        live = [(int(o), int(m)) for o, m in c["segs"] if m]
        gaps = gaps_of(c["segs"], c["numel"])
        count["odd offset"] += any(o % 2 for o, _ in live)
        count["offset not a multiple of 8"] += any(o % 8 for o, _ in live)
        count["back to back"] += len(live) > 1 and 0 in gaps[1:-1]
        count["non-padding gap"] += (not c["gaps_pad"]) and any(g > 0 for g in gaps[1:-1])
        count["odd numel"] += c["numel"] % 2
        count["refused broadcast"] += c["bcast"] and not flat_coverable(c)
        count["accepted broadcast with remainder"] += \
            c["bcast"] and flat_coverable(c) and c["numel"] % 8 != 0
        count["weighted at N >= 129"] += c["weighted"] and c["n"] >= 129
        count["weighted at N = 128"] += c["weighted"] and c["n"] == 128
        count["gap >= 128"] += max(gaps) >= 128
        count["naninf"] += c["naninf"]
        assert c["numel"] < 60000 and c["n"] < 260
    print(count)
    for k in ("odd offset", "non-padding gap", "odd numel", "refused broadcast",
              "accepted broadcast with remainder", "weighted at N >= 129"):
        assert count[k] >= 5, (k, count)
    assert min(count.values()) >= 1, count
