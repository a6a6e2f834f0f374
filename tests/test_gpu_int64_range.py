"""int64 keys over the range of the type, through every place the
``.float() -> mean -> copy_`` arithmetic lives: the direct int64 loads and
the packed-column staging of the default order, the torch-GPU-order paths,
the int64 bucket of a 16-bit launch and the stateless entry point.  Values
(tests/i64range.py): .float() ties at and above 2^24, the 2^31 / 2^32
boundary (a kernel reading the low word only passes every other test),
2^40, 2^53 + 1 and the largest powers of two whose n-fold sum stays in
range, both signs; bit for bit against oracle.torch_order.mean_i64_trunc
(pinned against torch's CPU arithmetic on the same values by
tests/test_oracle.py) and, in the torch-GPU order, torch's own cuda mean
followed by copy_.

Means of 2^63 or more in magnitude (INT64_MAX at n = 1) and NaN are left
out on purpose: torch's x86 copy_ gives INT64_MIN there, the device
conversion is not defined by the compiler, and include/fedagg.h says the
result is unspecified."""
import ctypes

import numpy as np
import pytest
import torch

import i64range as R
from feddct_amd import _lib
from oracle import torch_order as T

pytestmark = pytest.mark.gpu

GUARD = 64
G64 = -0x0123456789abcdef


class Bufs64:
    """n int64 client buckets and the result bucket, each between guards."""

    def __init__(self, x):
        self.n, self.numel = x.shape
        self.x = x
        self.row = self.numel + 2 * GUARD
        h = np.full((self.n, self.row), G64, np.int64)
        h[:, GUARD:GUARD + self.numel] = x
        self.c64 = torch.from_numpy(h).cuda()
        self.o64 = torch.full((self.row,), G64, dtype=torch.int64, device="cuda")
        self.a64 = _lib.ptr_array([self.c64.data_ptr() + 8 * (self.row * i + GUARD)
                                   for i in range(self.n)])
        self.p64 = self.o64.data_ptr() + 8 * GUARD

    def out(self):
        return self.o64.cpu().numpy()[GUARD:GUARD + self.numel]

    def assert_untouched(self, what):
        o = self.o64.cpu().numpy()
        assert (o[:GUARD] == G64).all() and (o[GUARD + self.numel:] == G64).all(), (what, "out64")
        c = self.c64.cpu().numpy()
        assert (c[:, :GUARD] == G64).all() and (c[:, GUARD + self.numel:] == G64).all(), what
        assert np.array_equal(c[:, GUARD:GUARD + self.numel], self.x), (what, "wrote a client")


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def want_cpu_order(x):
    return np.concatenate([T.mean_i64_trunc(x[:, o:o + m]) for o, m in R.SEGS64])


def check(got, want, x, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]], x[:, bad[:5]])


@pytest.mark.parametrize("n", R.NS)
def test_default_order_over_the_range(n):
    x = R.values(n)
    b = Bufs64(x)
    plan = _lib.Plan((), 0, R.SEGS64, R.NUMEL)
    rc = _lib.lib.fa_reduce(plan.handle, None, b.a64, n, None, None, b.p64, 0, stream())
    torch.cuda.synchronize()
    assert rc == _lib.FA_OK, _lib.lib.fa_last_error()
    want = want_cpu_order(x)
    if n == 1:      # .float() of the edges of the range, converted back
        assert {-2 ** 63, 2 ** 63 - 2 ** 39} <= set(want.tolist())
    check(b.out(), want, x, ("default", n))
    b.assert_untouched(n)


@pytest.mark.parametrize("n", R.NS)
def test_stateless_mean_i64_trunc_over_the_range(n):
    x = R.values(n, seed=1)
    b = Bufs64(x)
    segs, ns = _lib.seg_array(np.array(R.SEGS64, np.int64))
    rc = _lib.lib.fa_mean_i64_trunc(b.a64, n, R.NUMEL, b.p64, segs, ns, stream())
    torch.cuda.synchronize()
    assert rc == _lib.FA_OK, _lib.lib.fa_last_error()
    check(b.out(), want_cpu_order(x), x, ("stateless", n))
    b.assert_untouched(n)


def tgpu_ns():
    return [n for n in R.NS
            if all(_lib.lib.fa_torch_gpu_config(n, m, None) for m in R.KEYS)]


def test_torch_gpu_order_over_the_range():
    """Against torch's own cuda stack(...).float().mean(0) copied into an
    int64 tensor, per key, at the client counts fa_torch_gpu_config accepts
    for every key (the others have no torch-GPU-order plan to run)."""
    ns = tgpu_ns()
    assert len(ns) >= 4 and max(ns) >= 33, ns
    for n in ns:
        tgpu_case(n)


def tgpu_case(n):
    x = R.values(n, seed=2)
    b = Bufs64(x)
    plan = _lib.Plan((), 0, R.SEGS64, R.NUMEL, order=_lib.FA_ORDER_TORCH_GPU, n=n)
    rc = _lib.lib.fa_reduce(plan.handle, None, b.a64, n, None, None, b.p64, 0, stream())
    torch.cuda.synchronize()
    assert rc == _lib.FA_OK, _lib.lib.fa_last_error()
    dev = torch.from_numpy(x).cuda()
    want = torch.zeros(R.NUMEL, dtype=torch.int64, device="cuda")
    for o, m in R.SEGS64:
        ref = torch.stack([dev[i, o:o + m].float() for i in range(n)], 0).mean(0)
        want[o:o + m].copy_(ref)
    check(b.out(), want.cpu().numpy(), x, ("torch-gpu", n))
    b.assert_untouched(n)


def test_int64_bucket_of_a_16_bit_launch():
    """A bf16 plan at n = 9: the int64 columns ride in the 16-bit kernels'
    launch (fedagg_h16.hip), with their own loads and conversion."""
    n = 9
    x = R.values(n, seed=3)
    b = Bufs64(x)
    plan = _lib.Plan(np.array([[0, 40]]), 40, R.SEGS64, R.NUMEL, elem=_lib.FA_ELEM_BF16)
    c16 = torch.ones(n, 64, dtype=torch.bfloat16, device="cuda")
    o16 = torch.zeros(GUARD + 40 + GUARD, dtype=torch.bfloat16, device="cuda")   # zeros: guards
    a16 = _lib.ptr_array([c16[i].data_ptr() for i in range(n)])
    rc = _lib.lib.fa_reduce(plan.handle, a16, b.a64, n, None, o16.data_ptr() + 2 * GUARD, b.p64, 0,
                            stream())
    torch.cuda.synchronize()
    assert rc == _lib.FA_OK, _lib.lib.fa_last_error()
    check(b.out(), want_cpu_order(x), x, ("bf16 plan", n))
    assert (o16[GUARD:GUARD + 40] == 1).all()
    assert (o16[:GUARD] == 0).all() and (o16[GUARD + 40:] == 0).all(), "out16 guards"
    assert (c16 == 1).all()
    b.assert_untouched(n)
