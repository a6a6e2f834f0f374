"""FedProx proximal-term kernels (csrc/prox.hip: prox_partials, prox_finish,
prox_grad) through the C ABI against a float64 reference computed on the host,
at bounds derived from the kernels' documented summation order: chunk edges,
the multi-batch LDS finish, the global-memory finish, every gradient flag and
both store policies with controlled prior contents, the write contract (gaps
between segments keep their bits), degenerate plans, non-finite norms
(torch's CPU norm backward for the semantics), the module level with frozen
sides, and the refusals."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

U = 2.0 ** -24          # fp32 unit roundoff (round to nearest)
CHUNK = 4096            # floats per prox_partials chunk (prox.hip kChunk)
LDS_WORDS = 16384       # prox_finish<true> when nchunks + 2 nseg + 1 <= this (64 KiB)
FIN_BATCH = 8192        # partials the LDS finish stages per pass (kFinBlk * kFinLoads)


# ------------------------------------------------------------ the bounds --
def norm_bound(c):
    """Relative bound of norms[k] for a segment of ``c`` chunks, to first
    order in u = 2^-24, from the order prox.hip documents.

    The sum of squares has only non-negative terms, so the relative errors of
    the roundings on the path of any one term add up, and the sum's relative
    error is at most the longest such path:
      2  the subtraction a-b (one rounding, doubled by the square),
      1  the square,
      16 in-lane adds (4 float4 per lane: 3 adds inside each, 1 into the
         accumulator),
      1  the scalar-tail add,
      6  wave shuffles (64 lanes),
      3  cross-wave adds (4 waves, the first onto 0 exact),
      ceil(c/64) + 6 in the finish (lane l: partials l, l+64, ...; then the
         shuffle tree).
    The square root halves a relative error and adds one rounding (sqrtf is
    correctly rounded in this build: no fast-math)."""
    depth = 2 + 1 + 16 + 1 + 6 + 3 + -(-int(c) // 64) + 6
    return (depth / 2 + 1) * U


def total_bound(chunks):
    """Relative bound of the total: the norms are non-negative, so the worst
    norm's bound plus the add depth of their sum by wave 0, ceil(nseg/64)
    in-lane adds and 6 shuffles."""
    nseg = len(chunks)
    worst = max((norm_bound(c) for c in chunks), default=0.0)
    return worst + (-(-nseg // 64) + 6) * U


GRAD_BOUND = 4 * U
"""The overwrite gradient fl(fl(fl(gout*alpha)/norms[k]) * fl(a-b)) has four
roundings: relative bound 4u against gout*alpha*(a-b)/norms[k] in float64
with the kernel's own fp32 norms[k].  An accumulating side adds one rounding
of the sum: |got - want| <= u |want| + 4u |d|."""


def _within(got, want, lim, what):
    """|got - want| <= lim elementwise in float64 (atol 0: the inputs stay out
    of the denormal range); prints the worst error, as a fraction of its limit,
    first."""
    got = got.detach().cpu().double().reshape(-1)
    want = want.reshape(-1)
    lim = torch.as_tensor(lim, dtype=torch.float64)
    lim = lim.reshape(-1) if lim.numel() == want.numel() else lim.expand_as(want)
    err = (got - want).abs()
    nz = lim > 0
    if bool(nz.any()):
        i = int((err[nz] / lim[nz]).argmax())
        print(f"{what}: worst error {float((err[nz] / lim[nz])[i]):.3f} of its limit "
              f"({float(lim[nz][i] / want[nz][i].abs() / U):.1f} u)")
    bad = ~(err <= lim)
    assert not bool(bad.any()), (
        f"{what}: {int(bad.sum())} of {bad.numel()} beyond the bound; first at "
        f"{int(bad.nonzero()[0])}: got {float(got[bad][0])!r} want {float(want[bad][0])!r} "
        f"limit {float(lim[bad][0])!r}")


def _bits(x, y):
    return x.shape == y.shape and torch.equal(x.reshape(-1).view(torch.int32),
                                              y.reshape(-1).view(torch.int32))


# -------------------------------------------------------------- the plans --
class _Case:
    def __init__(self, segs, numel):
        from feddct_amd.prox import _NormPlan
        self.segs = np.asarray(segs, np.int64).reshape(-1, 2)
        self.numel = int(numel)
        with torch.cuda.device(DEV):
            self.plan = _NormPlan(self.segs, self.numel)
        self.nseg = len(self.segs)
        self.chunks = [-(-int(m) // CHUNK) for _, m in self.segs]
        self.nchunks = sum(self.chunks)
        self.lds_finish = self.nchunks + 2 * self.nseg + 1 <= LDS_WORDS

    def inside(self):
        m = torch.zeros(self.numel, dtype=torch.bool)
        for o, n in self.segs:
            m[o:o + n] = True
        return m


def _place(lengths, lead=8):
    """Segments of the given lengths at offsets that are multiples of 4, with
    gaps of 4 to 11 floats between them, 8 in front and 8 behind."""
    segs, off = [], lead
    for k, n in enumerate(lengths):
        segs.append((off, n))
        off = -(-(off + n + 4) // 4) * 4 + 4 * (k % 2)
    return np.array(segs, np.int64), off + 8


# the issue's lengths, plus 6 and 7: 23 chunks (no multiple of 2, 3 or 4, so
# every chunks-per-workgroup setting ends on a partly filled workgroup)
EDGE_LENGTHS = [1, 2, 3, 4, 5, 1023, 1024, 0, 1025, 4095, 4096, 4097, 8191, 8193,
                3 * 4096 + 7, 6, 7]
ZERO_SEG = 6     # index of the segment with a == b (length 1024)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _norms(case, a, b, reps=1):
    from feddct_amd import _lib
    outs = []
    for _ in range(reps):
        norms = torch.full((max(1, case.nseg),), -1.0, device=DEV)
        total = torch.full((), -1.0, device=DEV)
        _lib.check(_lib.lib.fa_prox_norms(case.plan.handle, a.data_ptr(), b.data_ptr(),
                                          norms.data_ptr(), total.data_ptr(), _stream()))
        outs.append((norms, total))
    torch.cuda.synchronize()
    return outs


def _ref_norms(segs, a, b):
    """float64 on the host: norm_k = sqrt(sum((a-b)^2)), total = sum(norm_k)."""
    d = a.cpu().double() - b.cpu().double()
    sq = d * d
    n = torch.zeros(len(segs), dtype=torch.float64)
    for k, (o, m) in enumerate(segs):
        n[k] = sq[o:o + m].sum().sqrt()
    return n, n.sum()


def _check_norms(case, a, b, out, what, only=None):
    norms, total = out
    want, want_total = _ref_norms(case.segs, a, b)
    lim = torch.tensor([norm_bound(c) for c in case.chunks], dtype=torch.float64) * want
    if only is not None:   # some segments only (the total is judged by the caller)
        _within(norms[only], want[only], lim[only], what + " norms")
        return
    _within(norms[:case.nseg], want, lim, what + " norms")
    _within(total, want_total, total_bound(case.chunks) * want_total, what + " total")


def _grad(case, a, b, norms, gout, alpha, prior_a, prior_b, flags=0, with_gb=True, policy=0,
          ex=True):
    """One fa_prox_grad(_ex) launch onto copies of the prior contents."""
    from feddct_amd import _lib
    ga, gb = prior_a.clone(), prior_b.clone()
    old = _lib.lib.fa_tune_prox_store(policy)
    assert old >= 0
    try:
        args = (case.plan.handle, a.data_ptr(), b.data_ptr(), norms.data_ptr(), gout.data_ptr(),
                alpha, ga.data_ptr(), gb.data_ptr() if with_gb else None)
        if ex:
            _lib.check(_lib.lib.fa_prox_grad_ex(*args, flags, _stream()))
        else:
            _lib.check(_lib.lib.fa_prox_grad(*args, _stream()))
        torch.cuda.synchronize()
    finally:
        _lib.lib.fa_tune_prox_store(old)
    return ga, gb


def _ref_d(case, a, b, norms, gout, alpha):
    """float64 on the host, given the kernel's own fp32 norms:
    gout*alpha*(a-b)/norms[k], 0 where norms[k] == 0 and outside segments."""
    diff = a.cpu().double() - b.cpu().double()
    nk = norms.cpu().double()
    s = float(gout.cpu().double()) * float(alpha)
    d = torch.zeros(case.numel, dtype=torch.float64)
    for k, (o, m) in enumerate(case.segs):
        if m and float(nk[k]) != 0.0:
            d[o:o + m] = s * diff[o:o + m] / nk[k]
    return d


def _check_grad(case, d, ga, gb, prior_a, prior_b, flags, with_gb, what):
    """Both buckets against the float64 model, and every element outside the
    segments (and all of B when grad_b was NULL) still the prior bits."""
    from feddct_amd import _lib
    acc_a = bool(flags & (_lib.FA_PROX_ACCUMULATE | _lib.FA_PROX_ACCUMULATE_A))
    acc_b = bool(flags & (_lib.FA_PROX_ACCUMULATE | _lib.FA_PROX_ACCUMULATE_B))
    inside = case.inside()
    pa, pb = prior_a.cpu(), prior_b.cpu()
    ga, gb = ga.cpu(), gb.cpu()
    for side, got, prior, acc, sign in (("A", ga, pa, acc_a, 1.0), ("B", gb, pb, acc_b, -1.0)):
        outside = ~inside if (side == "A" or with_gb) else torch.ones_like(inside)
        assert _bits(got[outside], prior[outside]), f"{what}: grad_{side.lower()} gap written"
        if side == "B" and not with_gb:
            continue
        if acc:
            want = prior.double() + sign * d
            lim = U * want.abs() + GRAD_BOUND * d.abs()
        else:
            want = sign * d
            lim = GRAD_BOUND * d.abs()
        _within(got[inside], want[inside], lim[inside], f"{what} grad_{side.lower()}")


@pytest.fixture(scope="module")
def edge():
    """The chunk-edge plan (case 1), its inputs (a near b, one zero norm), its
    norms at the default setting and random prior gradient contents; shared,
    never modified."""
    segs, numel = _place(EDGE_LENGTHS)
    case = _Case(segs, numel)
    assert case.nchunks == 23 and case.lds_finish
    gaps = segs[1:, 0] - (segs[:-1, 0] + segs[:-1, 1])
    assert (segs[:, 0] % 4 == 0).all() and gaps.min() >= 4 and gaps.max() <= 12
    g = torch.Generator(device=DEV).manual_seed(21)
    b = torch.randn(numel, device=DEV, generator=g)
    a = b + 0.01 * torch.randn(numel, device=DEV, generator=g)
    o, m = segs[ZERO_SEG]
    a[o:o + m] = b[o:o + m]
    (norms, total), = _norms(case, a, b)
    prior_a = torch.randn(numel, device=DEV, generator=g)
    prior_b = torch.randn(numel, device=DEV, generator=g)
    return case, a, b, norms, total, prior_a, prior_b


def _gout(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


# ------------------------------------------------------ 1. chunk edges --
@pytest.mark.parametrize("near", [True, False])
def test_edge_norms_match_float64(edge, near):
    """Lengths 1..5, 1,023..1,025, 4,095..4,097, 8,191, 8,193, 3*4,096+7 and
    an empty segment: norms and total within the derived bound, a zero norm
    exactly +0; with a near b and with independent a and b."""
    case, a, b, norms, total = edge[:5]
    if not near:
        g = torch.Generator(device=DEV).manual_seed(22)
        a = torch.randn(case.numel, device=DEV, generator=g)
        (norms, total), = _norms(case, a, b)
    else:
        assert _bits(norms[ZERO_SEG], torch.zeros((), device=DEV))
    assert _bits(norms[EDGE_LENGTHS.index(0)], torch.zeros((), device=DEV))
    _check_norms(case, a, b, (norms, total), "edges")


@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("accumulate", [False, True])
def test_edge_gradients_and_write_contract(edge, accumulate, policy):
    """Both gradients within bound on the chunk-edge plan, and every element
    outside the segments keeps its prior bits: overwrite (fa_prox_grad) and
    accumulate forms, both store policies."""
    from feddct_amd import _lib
    case, a, b, norms, _, pa, pb = edge
    gout = _gout(0.7)
    flags = _lib.FA_PROX_ACCUMULATE if accumulate else 0
    ga, gb = _grad(case, a, b, norms, gout, 1.0, pa, pb, flags, policy=policy, ex=accumulate)
    d = _ref_d(case, a, b, norms, gout, 1.0)
    _check_grad(case, d, ga, gb, pa, pb, flags, True, f"edges acc={accumulate} sp={policy}")
    if not accumulate:   # a zero norm: zeros, not 0/0
        o, m = case.segs[ZERO_SEG]
        assert not bool(ga[o:o + m].any()) and not bool(gb[o:o + m].any())


def test_edge_chunks_per_workgroup_same_bits(edge):
    """23 chunks at 1 to 4 chunks per workgroup (the last workgroup partly
    filled at 2, 3 and 4): norms and total the same bits as the default."""
    from feddct_amd import _lib
    case, a, b, norms, total = edge[:5]
    for cpw in (1, 2, 3, 4):
        old = _lib.lib.fa_tune_prox_cpw(cpw)
        assert old >= 0
        try:
            (n, t), = _norms(case, a, b)
        finally:
            _lib.lib.fa_tune_prox_cpw(old)
        assert _bits(n, norms) and _bits(t, total), cpw


# --------------------------------------------- 2. multi-batch LDS finish --
def test_lds_finish_more_than_one_load_batch():
    """2,750 segments of 8,193 floats: 8,250 chunks > 8,192, so the LDS finish
    (8,250 + 5,501 words <= 16,384) stages its partials in two passes; nseg >
    1,024, so the boundaries' second staging loop and the waves' wrap run."""
    nseg, n, stride = 2750, 8193, 8196
    case = _Case([(k * stride, n) for k in range(nseg)], nseg * stride)
    assert case.nchunks == 8250 > FIN_BATCH and case.lds_finish
    g = torch.Generator(device=DEV).manual_seed(23)
    b = torch.randn(case.numel, device=DEV, generator=g)
    a = b + 0.01 * torch.randn(case.numel, device=DEV, generator=g)
    outs = _norms(case, a, b, reps=2)
    assert _bits(outs[1][0], outs[0][0]) and _bits(outs[1][1], outs[0][1])
    d = (a.cpu().double() - b.cpu().double()).view(nseg, stride)[:, :n]
    want = (d * d).sum(1).sqrt()
    _within(outs[0][0], want, norm_bound(3) * want, "two-batch norms")
    _within(outs[0][1], want.sum(), total_bound(case.chunks) * want.sum(), "two-batch total")


# ------------------------------------------ 3. global-memory finish --
def test_global_finish_many_small_segments():
    """6,000 segments of 5 floats at stride 8: 6,000 + 12,001 words > 16,384,
    so prox_finish<false> reads partials, boundaries and (for the total) the
    norms it has just written from global memory."""
    nseg = 6000
    case = _Case([(8 * k, 5) for k in range(nseg)], 8 * nseg)
    assert case.nchunks == 6000 and not case.lds_finish
    g = torch.Generator(device=DEV).manual_seed(24)
    a = torch.randn(case.numel, device=DEV, generator=g)
    b = torch.randn(case.numel, device=DEV, generator=g)
    outs = _norms(case, a, b, reps=2)
    assert _bits(outs[1][0], outs[0][0]) and _bits(outs[1][1], outs[0][1])
    _check_norms(case, a, b, outs[0], "global finish")


# ------------------- 4. global-memory finish against the LDS finish --
def test_global_finish_same_bits_as_lds_finish(edge):
    """The chunk-edge plan with 8,200 empty segments appended takes
    prox_finish<false> (23 + 2*8,217 + 1 words); empty segments add no chunk
    and +0 norms, so the real segments' norms and the total are the LDS
    finish's bits.  With the empty segments interleaved the segments move
    across waves and lanes: the norms are still the same bits, the total
    (another lane assignment) is judged against float64."""
    case, a, b, norms, total = edge[:5]
    real = [tuple(s) for s in case.segs]
    tail = _Case(real + [(0, 0)] * 8200, case.numel)
    assert tail.nchunks == case.nchunks and not tail.lds_finish
    (n2, t2), = _norms(tail, a, b)
    assert torch.equal(n2[:case.nseg], norms) and _bits(n2[:case.nseg], norms)
    assert not bool(n2[case.nseg:].view(torch.int32).any())   # +0, every one
    assert torch.equal(t2, total) and _bits(t2, total)

    mixed, where = [], []
    for s in real:
        where.append(len(mixed))
        mixed += [s] + [(0, 0)] * 483
    inter = _Case(mixed, case.numel)
    assert inter.nchunks == case.nchunks and not inter.lds_finish and inter.nseg >= 8217
    (n3, t3), = _norms(inter, a, b)
    assert torch.equal(n3[where], norms) and _bits(n3[where], norms)
    assert int(n3.view(torch.int32).count_nonzero()) == int(norms.view(torch.int32).count_nonzero())
    _, want_total = _ref_norms(case.segs, a, b)
    _within(t3, want_total, total_bound(inter.chunks) * want_total, "interleaved total")


# --------------------------------------------------- 5. degenerate plans --
@pytest.mark.parametrize("segs", [[], [(0, 0), (4, 0), (8, 0), (64, 0), (128, 0)]],
                         ids=["nseg0", "all_empty"])
def test_degenerate_plans(segs):
    """nseg == 0 and a plan of empty segments only (the finish runs with no
    partials): total 0, norms +0 (none written for nseg == 0), the gradient
    launch a no-op."""
    case = _Case(segs, 128)
    assert case.nchunks == 0
    g = torch.Generator(device=DEV).manual_seed(25)
    a = torch.randn(128, device=DEV, generator=g)
    b = torch.randn(128, device=DEV, generator=g)
    (norms, total), = _norms(case, a, b)
    assert _bits(total, torch.zeros((), device=DEV))
    if case.nseg == 0:
        assert _bits(norms, torch.full((1,), -1.0, device=DEV))
    else:
        assert not bool(norms.view(torch.int32).any())
    pa = torch.randn(128, device=DEV, generator=g)
    pb = torch.randn(128, device=DEV, generator=g)
    for ex, flags in ((False, 0), (True, 1)):
        ga, gb = _grad(case, a, b, norms, _gout(0.7), 1.0, pa, pb, flags, ex=ex)
        assert _bits(ga, pa) and _bits(gb, pb)


# ----------------------------------------------------- 6. gradient flags --
@pytest.mark.parametrize("with_gb", [True, False], ids=["gb", "gb_null"])
@pytest.mark.parametrize("flags", [0, 2, 4, 6, 1], ids=["none", "A", "B", "A|B", "ACC"])
def test_grad_flags_alpha_gout_and_store_policy(edge, flags, with_gb):
    """Every accumulate flag, with grad_b given and NULL, alpha in {1, -0.5,
    0}, gout in {0.7, -3}, onto random prior contents: the float64 model,
    the gaps (and all of B when grad_b is NULL) untouched, ACCUMULATE the
    same bits as A|B, the sc1 store policy the same bits as the default."""
    case, a, b, norms, _, pa, pb = edge
    for gv in (0.7, -3.0):
        gout = _gout(gv)
        for alpha in (1.0, -0.5, 0.0):
            what = f"flags={flags} gb={with_gb} alpha={alpha} gout={gv}"
            ga, gb = _grad(case, a, b, norms, gout, alpha, pa, pb, flags, with_gb)
            d = _ref_d(case, a, b, norms, gout, alpha)
            _check_grad(case, d, ga, gb, pa, pb, flags, with_gb, what)
            ga1, gb1 = _grad(case, a, b, norms, gout, alpha, pa, pb, flags, with_gb, policy=1)
            assert _bits(ga1, ga) and _bits(gb1, gb), what + ": store policy 1 differs"
            if flags == 1:
                ga6, gb6 = _grad(case, a, b, norms, gout, alpha, pa, pb, 6, with_gb)
                assert _bits(ga6, ga) and _bits(gb6, gb), what + ": ACCUMULATE != A|B"
            if flags == 0:   # fa_prox_grad is fa_prox_grad_ex with no flag
                ga0, gb0 = _grad(case, a, b, norms, gout, alpha, pa, pb, 0, with_gb, ex=False)
                assert _bits(ga0, ga) and _bits(gb0, gb), what


# ------------------------------------------------ 7. non-finite norms --
def _torch_cpu_loop(case, a, b, scale):
    """The reference's loop body, (w - w_t).norm(2) and its backward, per
    segment with torch on the CPU in fp32: for the semantics of non-finite
    norms (which elements are NaN, which are 0), not for the digits."""
    a, b = a.cpu(), b.cpu()
    norms, ga, gb = [], torch.zeros(case.numel), torch.zeros(case.numel)
    for o, m in case.segs:
        w = a[o:o + m].clone().requires_grad_(True)
        w_t = b[o:o + m].clone().requires_grad_(True)
        n = (w - w_t).norm(2)
        (n * scale).backward()
        norms.append(n.detach())
        ga[o:o + m], gb[o:o + m] = w.grad, w_t.grad
    return torch.stack(norms), ga, gb


def _nonfinite_case(poison):
    segs, numel = _place([5, 8193, 1025, 4097])
    case = _Case(segs, numel)
    g = torch.Generator(device=DEV).manual_seed(26)
    b = torch.randn(numel, device=DEV, generator=g)
    a = b + 0.01 * torch.randn(numel, device=DEV, generator=g)
    o = int(segs[1, 0])
    poison(a, o)
    (norms, total), = _norms(case, a, b)
    gout = _gout(0.7)
    sent = torch.full((numel,), 7.0, device=DEV)
    ga, gb = _grad(case, a, b, norms, gout, 1.0, sent, sent, ex=False)
    t_norms, t_ga, t_gb = _torch_cpu_loop(case, a, b, float(gout))
    # the other segments: unaffected, and within bound
    others = [0, 2, 3]
    _check_norms(case, a, b, (norms, total), "other segments", only=others)
    d = _ref_d(case, a, b, norms, gout, 1.0)
    rest = case.inside()
    rest[o:o + 8193] = False
    _within(ga.cpu()[rest], d[rest], GRAD_BOUND * d[rest].abs(), "other segments grad_a")
    _within(gb.cpu()[rest], -d[rest], GRAD_BOUND * d[rest].abs(), "other segments grad_b")
    seg = slice(o, o + 8193)
    return norms.cpu(), total.cpu(), ga.cpu()[seg], gb.cpu()[seg], t_norms, t_ga[seg], t_gb[seg]


def test_nan_norm_gives_nan_gradients_as_torch():
    """One NaN element in a three-chunk segment: torch's norm backward masks
    only norm == 0, so the segment's norm, the total and every gradient
    element of that segment are NaN on both sides; so must the kernel's be."""
    def poison(a, o):
        a[o + 3] = float("nan")
    norms, total, ga, gb, t_norms, t_ga, t_gb = _nonfinite_case(poison)
    assert bool(t_norms[1].isnan()) and bool(t_ga.isnan().all()) and bool(t_gb.isnan().all())
    assert bool(norms[1].isnan()) and bool(total.isnan())
    assert bool(ga.isnan().all()), f"{int((~ga.isnan()).sum())} grad_a elements not NaN"
    assert bool(gb.isnan().all()), f"{int((~gb.isnan()).sum())} grad_b elements not NaN"


def test_overflowed_norm_gives_zero_gradients_as_torch():
    """Elements near 3e38 in every chunk of a segment: the squares overflow,
    the norm and the total are inf, and the gradients are 0 on both sides
    (finite / inf), as torch gives."""
    def poison(a, o):
        for j, i in enumerate((0, 1, 2, 3, 4100, 4101, 8191, 8192)):
            a[o + i] = 3e38 * (1 + 0.01 * j)
    norms, total, ga, gb, t_norms, t_ga, t_gb = _nonfinite_case(poison)
    assert float(t_norms[1]) == math.inf and not bool(t_ga.any()) and not bool(t_gb.any())
    assert float(norms[1]) == math.inf and float(total) == math.inf
    assert not bool(ga.any()) and not bool(gb.any())


# ------------------------------------- 8. module level, frozen sides --
def _prox_models(seed):
    torch.manual_seed(seed)
    mk = lambda: torch.nn.Sequential(torch.nn.Conv2d(3, 16, 3), torch.nn.BatchNorm2d(16),  # noqa
                                     torch.nn.Conv2d(16, 33, 3, bias=False), torch.nn.Linear(7, 5)).to(DEV)
    return mk(), mk()


@pytest.mark.parametrize("flat", [False, True], ids=["per_param", "flat_grads"])
@pytest.mark.parametrize("frozen", ["global", "client", "none"])
def test_proximal_term_frozen_sides(frozen, flat):
    """proximal_term with the global's parameters frozen (the reference's
    practical case: grad_b NULL), the client's frozen (the scratch target) and
    neither, against the reference loop under float64 CPU autograd on copies.
    The gradients there divide by the float64 norm, not the kernel's fp32 one,
    so their bound is the gradient's 4u plus the norm's own bound for the
    parameter's chunk count.  A frozen side's .grad stays None."""
    from feddct_amd.prox import proximal_term
    c, g = _prox_models(31)
    scale = float(np.float32(0.37))
    refs = []
    for model, name in ((c, "client"), (g, "global")):
        for p in model.parameters():
            p.requires_grad_(frozen != name)
        refs.append([p.detach().cpu().double().requires_grad_(frozen != name)
                     for p in model.parameters()])
    pt = 0.0
    for w, w_t in zip(*refs):
        pt = pt + (w - w_t).norm(2)
    (pt * scale).backward()
    got = proximal_term(c, g, flat_grads=flat)
    (got * 0.37).backward()
    torch.cuda.synchronize()
    chunks = [-(-p.numel() // CHUNK) for p in c.parameters()]
    _within(got, pt.detach(), total_bound(chunks) * abs(float(pt)), f"term frozen={frozen}")
    for model, ref, name in ((c, refs[0], "client"), (g, refs[1], "global")):
        for (n, p), r, ch in zip(model.named_parameters(), ref, chunks):
            if frozen == name:
                assert p.grad is None and r.grad is None, n
            else:
                _within(p.grad, r.grad, (GRAD_BOUND + norm_bound(ch)) * r.grad.abs(),
                        f"{name} {n} frozen={frozen} flat={flat}")


# ------------------------------------------------------------ 9. refusals --
def test_refusals_launch_nothing(edge):
    from feddct_amd import _lib
    lib = _lib.lib
    case, a, b, norms, _, pa, pb = edge
    h = ctypes.c_void_p()
    arr, n = _lib.seg_array(np.array([(0, 8), (10, 4)], np.int64))
    assert lib.fa_norm_plan_create(arr, n, 64, ctypes.byref(h)) == _lib.FA_E_ALIGN and not h.value
    arr, n = _lib.seg_array(np.array([(0, 8), (60, 5)], np.int64))
    assert lib.fa_norm_plan_create(arr, n, 64, ctypes.byref(h)) == _lib.FA_E_INVAL and not h.value

    # room for a bucket that starts 4 bytes in
    a1 = torch.zeros(case.numel + 4, device=DEV)
    n_out = torch.full((case.nseg,), -1.0, device=DEV)
    t_out = torch.full((), -1.0, device=DEV)
    st = _stream()
    for pa_, pb_ in ((a1.data_ptr() + 4, b.data_ptr()), (a.data_ptr(), a1.data_ptr() + 4)):
        assert lib.fa_prox_norms(case.plan.handle, pa_, pb_, n_out.data_ptr(), t_out.data_ptr(),
                                 st) == _lib.FA_E_ALIGN
    ga, gb = pa.clone(), pb.clone()
    gout = _gout(0.7)
    good = [a.data_ptr(), b.data_ptr(), ga.data_ptr(), gb.data_ptr()]
    for i in range(4):
        p = list(good)
        p[i] = a1.data_ptr() + 4
        assert lib.fa_prox_grad_ex(case.plan.handle, p[0], p[1], norms.data_ptr(), gout.data_ptr(),
                                   1.0, p[2], p[3], 0, st) == _lib.FA_E_ALIGN, i
        assert lib.fa_prox_grad(case.plan.handle, p[0], p[1], norms.data_ptr(), gout.data_ptr(),
                                1.0, p[2], p[3], st) == _lib.FA_E_ALIGN, i
    assert lib.fa_prox_grad_ex(case.plan.handle, *good[:2], norms.data_ptr(), gout.data_ptr(), 1.0,
                               *good[2:], 8, st) == _lib.FA_E_INVAL
    assert lib.fa_prox_grad_ex(case.plan.handle, *good[:2], norms.data_ptr(), gout.data_ptr(), 1.0,
                               *good[2:], 1 | 16, st) == _lib.FA_E_INVAL
    assert lib.fa_tune_prox_cpw(5) == _lib.FA_E_INVAL
    assert lib.fa_tune_prox_cpw(0) == 0      # the refused setting was not kept
    torch.cuda.synchronize()
    assert _bits(n_out, torch.full_like(n_out, -1.0)) and _bits(t_out, torch.full_like(t_out, -1.0))
    assert _bits(ga, pa) and _bits(gb, pb) and not bool(a1.any())
