"""The 16-bit proximal term without a GPU: the new C-ABI symbols are exported
and bound and refuse NULL arguments and unsupported element pairs, and the
tests' restatement of the definition (tests/prox16ref.py) is what CPU torch
computes for the reference's loop — gradients and the running 16-bit total
bit for bit, for fp16 and bf16, and the dtypes of an fp32 master global over a
16-bit client."""
import numpy as np
import pytest
import torch

import prox16ref as P

TORCH_DT = {"float16": torch.float16, "bfloat16": torch.bfloat16}


def _t(bits, dtype):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(TORCH_DT[dtype])


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.int16).numpy().view(np.uint16)


# ------------------------------------------------------------- the ABI ----
def test_new_symbols_exported_and_bound():
    from feddct_amd import _lib
    for name, nargs in (("fa_prox_norms_elem", 8), ("fa_prox_grad_elem", 12)):
        assert name in _lib.EXPORTS
        fn = getattr(_lib.lib, name)
        assert len(fn.argtypes) == nargs and fn.restype is _lib._I


def test_null_and_bad_pairs_refused_without_a_gpu():
    from feddct_amd import _lib
    L = _lib.lib
    F32, F16, BF16 = _lib.FA_ELEM_F32, _lib.FA_ELEM_F16, _lib.FA_ELEM_BF16
    good = [(F16, F16), (BF16, BF16), (F16, F32), (BF16, F32), (F32, F32)]
    bad = [(F32, F16), (F32, BF16), (F16, BF16), (BF16, F16), (3, 3), (-1, F32), (F16, 7)]
    for ae, be in good:   # a supported pair: the NULL arguments are what is refused
        assert L.fa_prox_norms_elem(None, None, ae, None, be, None, None, None) == _lib.FA_E_INVAL
        assert b"NULL" in L.fa_last_error(), (ae, be)
        assert L.fa_prox_grad_elem(None, None, ae, None, be, None, None, 1.0, None, None, 0,
                                   None) == _lib.FA_E_INVAL
        assert b"NULL" in L.fa_last_error(), (ae, be)
    for ae, be in bad:
        assert L.fa_prox_norms_elem(None, None, ae, None, be, None, None, None) == _lib.FA_E_INVAL
        assert b"pair" in L.fa_last_error(), (ae, be)
        assert L.fa_prox_grad_elem(None, None, ae, None, be, None, None, 1.0, None, None, 0,
                                   None) == _lib.FA_E_INVAL
        assert b"pair" in L.fa_last_error(), (ae, be)


# ------------------------------------------- the restatement against torch --
def _reference_loop(ws, wts, gout):
    """train_fedprox.py:113-115 with backward, on CPU torch."""
    proximal_term = 0.0
    for w, w_t in zip(ws, wts):
        proximal_term += (w - w_t).norm(2)
    proximal_term.backward(gout)
    return proximal_term.detach()


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_restatement_is_torch_cpu_bit_for_bit(dtype, seed):
    """The reference loop with backward() on CPU torch over the kernel tests'
    lengths: per parameter torch's 16-bit norm lies in the restated interval
    (equal to it where the interval is one value: at least 90 % of the
    segments), the gradients of both sides equal the restated
    rn16(gout16 * rn16(d16 / n16)) from torch's own norm, the term equals the
    restated in-order 16-bit running sum of torch's norms, and a second
    backward accumulates as rn16(old + new) — all bit for bit."""
    segs, numel = P.place(P.LENGTHS)
    a, b = P.inputs(numel, seed, dtype, same=[tuple(segs[P.ZERO_SEG])])
    exact, live, iv = P.exact_share(segs, a, b, dtype)
    print(f"{dtype} seed {seed}: {exact} of {live} norms determined")
    assert exact >= 0.9 * live
    ws = [_t(a[o:o + m], dtype).requires_grad_(True) for o, m in segs]
    wts = [_t(b[o:o + m], dtype).requires_grad_(True) for o, m in segs]
    gout = torch.tensor(0.7).to(TORCH_DT[dtype])
    gb = int(_bits(gout)[0])
    term = _reference_loop(ws, wts, gout)
    assert term.dtype == TORCH_DT[dtype] and term.dim() == 0
    norms = []
    for k, (w, w_t) in enumerate(zip(ws, wts)):
        with torch.no_grad():
            n = int(_bits((w - w_t).norm(2))[0])
        norms.append(n)
        lo, hi = iv[k]
        assert lo <= n <= hi, (k, lo, n, hi)   # (non-negative patterns order as values)
        d = P.diff16(_bits(w), _bits(w_t), dtype)
        assert np.array_equal(d, _bits(w.detach() - w_t.detach())), k
        want = P.grad16(d, n, gb, dtype)
        assert np.array_equal(_bits(w.grad), want), (k, "grad_w")
        assert np.array_equal(_bits(w_t.grad), P.neg16(want)), (k, "grad_w_t")
        assert w.grad.dtype == w_t.grad.dtype == TORCH_DT[dtype]
    assert norms[P.ZERO_SEG] == 0 and not _bits(ws[P.ZERO_SEG].grad).any()
    assert int(_bits(term)[0]) == P.running_total(norms, dtype)
    first = [_bits(w.grad).copy() for w in ws]
    _reference_loop(ws, wts, gout)
    for k, w in enumerate(ws):
        assert np.array_equal(_bits(w.grad), P.acc16(first[k], first[k], dtype)), k


@pytest.mark.parametrize("dtype,big,small_sum", [("bfloat16", 256.0, 320.0),
                                                 ("float16", 2048.0, 2112.0)])
def test_running_total_order_is_observable(dtype, big, small_sum):
    """One norm of 256 (bf16; 2048 in fp16) followed by 64 ones stays where it
    is; the ones first give 320 (2112): torch's loop and the restatement."""
    dt = TORCH_DT[dtype]
    vals = [big] + [1.0] * 64
    for order, want in ((vals, big), (vals[::-1], small_sum)):
        ws = [torch.tensor([v], dtype=dt) for v in order]
        wts = [torch.zeros(1, dtype=dt) for _ in order]
        t = 0.0
        for w, w_t in zip(ws, wts):
            t += (w - w_t).norm(2)
        assert float(t) == want
        nb = [int(_bits(w)[0]) for w in ws]
        assert P.running_total(nb, dtype) == int(_bits(t)[0])


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_mixed_pair_dtypes_and_client_gradient(dtype):
    """A 16-bit client against an fp32 global: w - w_t promotes, so the term
    and the global's gradient are fp32, the client's gradient has the client's
    dtype and is rn16 of the negated global gradient, bit for bit."""
    segs, numel = P.place(P.LENGTHS)
    a, b = P.inputs(numel, 3, dtype)
    rng = np.random.default_rng(4)
    ws = [_t(a[o:o + m], dtype).requires_grad_(True) for o, m in segs]
    wts = [torch.from_numpy(rng.standard_normal(m).astype(np.float32)).requires_grad_(True)
           for _, m in segs]
    term = _reference_loop(ws, wts, torch.tensor(0.7))
    assert term.dtype == torch.float32
    for k, (w, w_t) in enumerate(zip(ws, wts)):
        assert w.grad.dtype == TORCH_DT[dtype] and w_t.grad.dtype == torch.float32
        want = P.rn16((-w_t.grad).numpy(), dtype)
        assert np.array_equal(_bits(w.grad), want), k
