"""Shared by the tests of the striped multi-GPU round on fp16 / bf16 buckets
(test_round16_cpu.py, test_gpu_round16.py): the
layouts, client data as uint16 bit patterns, the oracle expectation, the
schedule replay on 16-bit buffers and the oracle arithmetic backend of
dist.StripedAggregator.

The expectation of a key is the reference's: every value widened exactly to
fp32, ``oracle.torch_order.torch_mean0`` (torch's CPU order), one rounding to
nearest-even into the 16-bit type (torch's own ``.to(dtype)``).
"""
import functools

import numpy as np
import torch

import schedsim
from feddct_amd.layout import BucketLayout
from oracle import torch_order as O
from test_distloop_cpu import MANS

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
ELEM = {"float16": 1, "bfloat16": 2}          # FA_ELEM_F16, FA_ELEM_BF16
FILL16 = 0xFFFF                               # a NaN in both types
LAYOUTS = ("A", "B", "C", "raw")


class RawLayout:
    """A raw 16-bit segment list with what comm.py / dist.py / partition.py
    read of a BucketLayout: a key at an offset that is no multiple of 8, a
    5-element key, a bucket length of residue 5 modulo 8; 128-aligned vector
    keys in between so that stripes can be cut."""
    native16 = True
    master16 = False

    def __init__(self, dtype):
        self.float_dtype = DTYPES[dtype]
        self.segs32 = np.array([(0, 2088), (2179, 300), (2560, 5), (2688, 4096), (6912, 2048),
                                (9000, 37), (9100, 1)], np.int64)
        self.f32_numel = 9133
        self.segs64 = np.array([(0, 1), (1, 3)], np.int64)
        self.i64_numel = 4
        self.signature = ("<raw16>", dtype)

    def __hash__(self):
        return hash(self.signature)

    def __eq__(self, other):
        return isinstance(other, RawLayout) and self.signature == other.signature


@functools.lru_cache(maxsize=None)
def layout_of(name, dtype):
    """Layouts A / B / C of tests/test_distloop_cpu.MANS cast to ``dtype`` and
    laid out natively, or the raw one."""
    if name == "raw":
        return RawLayout(dtype)
    return BucketLayout([(e["key"], e["shape"], e["dtype"] if e["dtype"] == "int64" else dtype)
                         for e in MANS[name]["keys"]], native16=True)


def fp32_layout_of(name):
    return BucketLayout.from_manifest(MANS[name])


# ------------------------------------------------------------ conversions --
def widen(bits, dtype):
    """uint16 patterns -> float32, exactly."""
    b = np.ascontiguousarray(bits, np.uint16)
    return torch.from_numpy(b.view(np.int16)).view(DTYPES[dtype]).float().numpy()


def narrow(x32, dtype):
    """float32 -> uint16 patterns, torch's round to nearest-even."""
    t = torch.from_numpy(np.ascontiguousarray(x32, np.float32)).to(DTYPES[dtype])
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def is_nan16(bits, dtype):
    b = np.asarray(bits, np.uint16)
    if dtype == "float16":
        return ((b & 0x7C00) == 0x7C00) & ((b & 0x03FF) != 0)
    return ((b & 0x7F80) == 0x7F80) & ((b & 0x007F) != 0)


def same16(got, want, dtype):
    """Bit for bit, two NaNs equal whatever their payload — but the fill's
    pattern in ``got`` is an element nobody wrote, unless expected so."""
    got, want = np.asarray(got, np.uint16), np.asarray(want, np.uint16)
    if got.shape != want.shape:
        return False
    both_nan = is_nan16(got, dtype) & is_nan16(want, dtype) & (got != FILL16)
    return bool(((got == want) | both_nan).all())


def as_tensor(bits, dtype, device="cpu"):
    """uint16 patterns as a tensor of ``dtype`` (a copy)."""
    b = np.ascontiguousarray(bits, np.uint16).copy()
    return torch.from_numpy(b.view(np.int16)).view(DTYPES[dtype]).to(device)


def bits_of(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


# -------------------------------------------------------------------- data --
def cancelling_bits(dtype, n, m, seed):
    """Cancellation-heavy rows: magnitudes 2^-12 .. 2^12 with full mantissas
    and random signs, so the result's bits depend on the summation order."""
    rng = np.random.default_rng([seed, n, m, ELEM[dtype]])
    x = np.ldexp(rng.uniform(1.0, 2.0, (n, m)), rng.integers(-12, 12, (n, m)))
    x *= rng.choice([-1.0, 1.0], (n, m))
    return narrow(x.astype(np.float32), dtype)


def clients16(name, dtype, n, seed):
    """(bits[n, f32_numel] uint16, i64[n, max(1, i64_numel)]) of n clients."""
    lay = layout_of(name, dtype)
    bits = cancelling_bits(dtype, n, lay.f32_numel, seed)
    rng = np.random.default_rng([seed, 64])
    i64 = rng.integers(-(1 << 40), 1 << 40, (n, max(1, lay.i64_numel))).astype(np.int64)
    i64[:, :1] = rng.integers(0, 1000, (n, 1))
    return bits, i64


def expected16(lay, dtype, bits, i64=None):
    """(expected uint16 [f32_numel], mask of the elements inside a segment,
    expected int64 [i64_numel] or None): the oracle over every client row."""
    exp = np.zeros(lay.f32_numel, np.uint16)
    inside = np.zeros(lay.f32_numel, bool)
    with np.errstate(all="ignore"):
        for o, m in lay.segs32:
            o, m = int(o), int(m)
            exp[o:o + m] = narrow(O.torch_mean0(widen(bits[:, o:o + m], dtype)), dtype)
            inside[o:o + m] = True
    e64 = None
    if i64 is not None and lay.i64_numel:
        e64 = np.zeros(lay.i64_numel, np.int64)
        for o, m in lay.segs64:
            o, m = int(o), int(m)
            e64[o:o + m] = O.mean_i64_trunc(i64[:, o:o + m])
    return exp, inside, e64


# ---------------------------------------------------------- schedule replay --
class Sim16(schedsim.Sim):
    """tests/schedsim.py on 16-bit buckets: the floating buffers the striped
    round touches (CLIENT, RECV, OUT, STRIPE) hold uint16 patterns, exchanges
    copy them raw, and the stripe kernel widens, sums in the oracle's column
    order, divides and rounds once."""

    def __init__(self, layout, dtype, tiles, counts, clients16_, clients64):
        super().__init__(layout, tiles, counts, clients16_, clients64)
        self.dtype = dtype
        n16 = layout.f32_numel
        for b in self.buf:
            b["OUT"] = np.full(n16, FILL16, np.uint16)
            b["STRIPE"] = np.full(n16, FILL16, np.uint16)
            b["RECV"] = schedsim.defaultdict(lambda: np.full(n16, FILL16, np.uint16))

    def _kernel(self, r, x):
        if x["op"] != "K_STRIPE":
            assert x["op"] in ("K_STACK", "K_TAILS"), x    # the int64 keys
            return super()._kernel(r, x)
        b = self.buf[r]
        mine = range(self.first[r], self.first[r] + self.counts[r])
        with np.errstate(all="ignore"):
            for st, cnt, kind in self._tiles_in(x["offset"], x["count"]):
                rows = [widen((self.c32[s] if s in mine else b["RECV"][s])[st:st + cnt],
                              self.dtype) for s in range(self.n)]
                res = (np.float32(0) + schedsim._column_sum(kind, rows)).astype(np.float32)
                b[x["dst"]][st:st + cnt] = narrow(res / np.float32(self.n), self.dtype)


# --------------------------------------------- dist.py's arithmetic backend --
class OracleStripeBackend16:
    """dist.StripedAggregator's backend on CPU tensors of a 16-bit dtype: a
    chunk's columns reduced per key range in the order the column needs
    (cascade over the key's body columns, ILP-4 over its tail, the M == 1
    rule), on the widened values, then rounded once."""

    def __init__(self, layout, dtype):
        self.layout, self.dtype = layout, dtype

    def reduce_chunk(self, c, lo, hi, sources, out32, weights=None):
        assert weights is None
        n = len(sources)
        for o, M in self.layout.segs32:
            o, M = int(o), int(M)
            a, b = max(o, lo), min(o + M, hi)
            if a >= b:
                continue
            x = np.stack([widen(bits_of(t[a - base:b - base]), self.dtype)
                          for t, base in sources])
            res = np.empty(b - a, np.float32)
            with np.errstate(all="ignore"):
                if M == 1:
                    col = x[:, 0]
                    res[0] = (O.ilp4([col[i:i + 1] for i in range(n)])[0] if n < 8
                              else O.inner8(col))
                else:
                    body = o + O.body_len(M)
                    k = min(max(body - a, 0), b - a)     # columns of [a, b) in the body
                    if k:
                        res[:k] = O.cascade([x[i, :k] for i in range(n)])
                    if k < b - a:
                        res[k:] = O.ilp4([x[i, k:] for i in range(n)])
                res = ((np.float32(0) + res).astype(np.float32) / np.float32(n)).astype(np.float32)
            out32[a:b] = as_tensor(narrow(res, self.dtype), self.dtype)

    def reduce_i64(self, clients64, out):
        for o, m in self.layout.segs64:
            o, m = int(o), int(m)
            x = np.stack([t[o:o + m].cpu().numpy() for t in clients64])
            out[o:o + m] = torch.from_numpy(O.mean_i64_trunc(x))


class SpecialLayout(RawLayout):
    """tests/specials.py's raw layout (every column rule under every special
    pattern), its offsets taken as 16-bit elements; no int64 keys."""

    def __init__(self, dtype):
        import specials
        super().__init__(dtype)
        segs, numel, _ = specials.layout()
        self.segs32, self.f32_numel = segs, int(numel)
        self.segs64, self.i64_numel = np.zeros((0, 2), np.int64), 0
        self.signature = ("<specials16>", dtype)
