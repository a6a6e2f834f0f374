"""The 16-bit proximal-term kernels (csrc/prox_h16.hip) through the C ABI
(fa_prox_norms_elem / fa_prox_grad_elem), for bf16 and fp16, pure (a 16-bit
global) and mixed (an fp32 master global): the norms inside the interval the
restated definition (tests/prox16ref.py) leaves to the fp32 summation order
(one value for at least 90 % of the segments), the 16-bit total bit-equal to
the in-order 16-bit running sum of the kernel's own norms (more than 64
segments, an order-sensitive case, the global-memory finish), the gradients
bit-equal to CPU torch's formula from the kernel's own norms, every accumulate
flag over known prior contents, the write contract (gaps and guard bands keep
their bits), repeats, non-finite norms and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import prox16ref as P
from test_gpu_prox_edges import GRAD_BOUND, U, norm_bound, total_bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TORCH_DT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
DTYPES = ["bfloat16", "float16"]
LDS_WORDS = 16384       # the LDS finish when nchunks + 2 nseg + 1 <= this


def _elem(dtype):
    from feddct_amd import _lib
    return {"float16": _lib.FA_ELEM_F16, "bfloat16": _lib.FA_ELEM_BF16,
            "float32": _lib.FA_ELEM_F32}[dtype]


def _t(bits, dtype, dev=DEV):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(
        TORCH_DT[dtype]).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.int16).numpy().view(np.uint16)


def _same(x, y):
    """Bit-equal tensors of one dtype (2- or 4-byte elements)."""
    iv = torch.int16 if x.element_size() == 2 else torch.int32
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(
        x.cpu().reshape(-1).view(iv), y.cpu().reshape(-1).view(iv))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Case:
    def __init__(self, segs, numel):
        from feddct_amd.prox import _NormPlan
        self.segs = np.asarray(segs, np.int64).reshape(-1, 2)
        self.numel, self.nseg = int(numel), len(self.segs)
        with torch.cuda.device(DEV):
            self.plan = _NormPlan(self.segs, self.numel)
        self.chunks = [-(-int(m) // P.CHUNK) for _, m in self.segs]
        self.lds_finish = sum(self.chunks) + 2 * self.nseg + 1 <= LDS_WORDS

    def inside(self):
        m = torch.zeros(self.numel, dtype=torch.bool)
        for o, n in self.segs:
            m[o:o + n] = True
        return m


def _norms(case, a, b, dtype, mixed):
    """One fa_prox_norms_elem launch into guard-filled outputs: (norms fp32
    [nseg + 2] with a guard on either side, total with its guard)."""
    from feddct_amd import _lib
    norms = torch.full((case.nseg + 2,), -7.0, device=DEV)
    tdt = torch.float32 if mixed else TORCH_DT[dtype]
    total = torch.full((3,), -7.0, device=DEV, dtype=tdt)
    _lib.check(_lib.lib.fa_prox_norms_elem(
        case.plan.handle, a.data_ptr(), _elem(dtype), b.data_ptr(),
        _elem("float32" if mixed else dtype), norms[1:].data_ptr(), total[1:].data_ptr(),
        _stream()), "fa_prox_norms_elem")
    torch.cuda.synchronize()
    assert float(norms[0]) == -7.0 and float(norms[-1]) == -7.0, "norms guard written"
    assert float(total[0]) == -7.0 and float(total[2]) == -7.0, "total guard written"
    return norms[1:1 + case.nseg].clone(), total[1].clone()


def _grad(case, a, b, dtype, mixed, norms, gout, alpha, prior_a, prior_b, flags=0, with_gb=True):
    from feddct_amd import _lib
    ga, gb = prior_a.clone(), prior_b.clone()
    _lib.check(_lib.lib.fa_prox_grad_elem(
        case.plan.handle, a.data_ptr(), _elem(dtype), b.data_ptr(),
        _elem("float32" if mixed else dtype), norms.data_ptr(), gout.data_ptr(), alpha,
        ga.data_ptr(), gb.data_ptr() if with_gb else None, flags, _stream()), "fa_prox_grad_elem")
    torch.cuda.synchronize()
    return ga, gb


def _torch_grad16(case, a, b, norms, gout, alpha, dt):
    """CPU torch, from the kernel's own norms: rn16(rn16(gout * alpha) *
    rn16(d16 / norms[k])), 0 where norms[k] == 0 and outside the segments."""
    d16 = a.cpu() - b.cpu()                       # rn16(fp32(a) - fp32(b))
    n = norms.cpu()
    gs = (gout.cpu().float() * alpha).to(dt)
    g = torch.zeros(case.numel, dtype=dt)
    for k, (o, m) in enumerate(case.segs):
        if m and float(n[k]) != 0.0:
            q = (d16[o:o + m].float() / n[k]).to(dt)
            g[o:o + m] = (gs.float() * q.float()).to(dt)
    return g


@pytest.fixture(scope="module", params=DTYPES)
def edge(request):
    """The edge plan, its inputs (one segment with a == b), the fp32 global of
    the mixed form, both forms' norms and random prior gradient contents;
    shared, never modified."""
    dtype = request.param
    dt = TORCH_DT[dtype]
    segs, numel = P.place(P.LENGTHS)
    gaps = segs[1:, 0] - (segs[:-1, 0] + segs[:-1, 1])
    assert (segs[:, 0] % 8 == 0).all() and gaps.min() >= 8 and gaps.max() <= 23
    ab, bb = P.inputs(numel, 0, dtype, same=[tuple(segs[P.ZERO_SEG])])
    case = _Case(segs, numel)
    assert case.lds_finish
    a, b = _t(ab, dtype), _t(bb, dtype)
    g = torch.Generator(device=DEV).manual_seed(41)
    b32 = b.float() + 0.001 * torch.randn(numel, device=DEV, generator=g)   # not 16-bit values
    o, m = segs[P.ZERO_SEG]
    b32[o:o + m] = a[o:o + m].float()
    prior = {"a": torch.randn(numel, device=DEV, generator=g).to(dt),
             "b": torch.randn(numel, device=DEV, generator=g).to(dt),
             "b32": torch.randn(numel, device=DEV, generator=g)}
    return dict(dtype=dtype, dt=dt, case=case, ab=ab, bb=bb, a=a, b=b, b32=b32, prior=prior,
                pure=_norms(case, a, b, dtype, False), mixed=_norms(case, a, b32, dtype, True))


# ------------------------------------------------------------- forward ----
def test_pure_norms_in_the_restated_interval(edge):
    """norms[k] is a 16-bit value inside [rn16(lo), rn16(hi)]; the interval is
    a single value for at least 90 % of the segments (asserted on the CPU
    first), so the check is exact there; a zero and an empty segment give +0;
    the total is the in-order 16-bit running sum of these norms."""
    dtype, case = edge["dtype"], edge["case"]
    exact, live, iv = P.exact_share(case.segs, edge["ab"], edge["bb"], dtype)
    print(f"{dtype}: {exact} of {live} norms determined")
    assert exact >= 0.9 * live
    norms, total = edge["pure"]
    nb = P.rn16(norms.cpu().numpy(), dtype)
    assert np.array_equal(P.f32(nb, dtype), norms.cpu().numpy()), "norms[] are not 16-bit values"
    for k, (lo, hi) in enumerate(iv):
        assert lo <= int(nb[k]) <= hi, (k, case.segs[k], hex(lo), hex(int(nb[k])), hex(hi))
    assert nb[P.ZERO_SEG] == 0 and nb[P.LENGTHS.index(0)] == 0
    assert int(_bits(total)[0]) == P.running_total(nb, dtype)
    n2, t2 = _norms(case, edge["a"], edge["b"], dtype, False)
    assert _same(n2, norms) and _same(t2, total), "a repeated launch gave other bits"


def test_mixed_norms_and_total_fp32_bounds(edge):
    """An fp32 global: prox.hip's fp32 bounds on fp32(a), against float64."""
    case = edge["case"]
    norms, total = edge["mixed"]
    assert total.dtype == torch.float32
    d = edge["a"].cpu().double() - edge["b32"].cpu().double()
    want = torch.stack([(d[o:o + m] ** 2).sum().sqrt() for o, m in case.segs])
    err = (norms.cpu().double() - want).abs()
    lim = torch.tensor([norm_bound(c) for c in case.chunks], dtype=torch.float64) * want
    print("mixed norms: worst", float((err / lim.clamp_min(1e-300)).max()), "of the limit")
    assert bool((err <= lim).all())
    assert float(norms[P.ZERO_SEG]) == 0.0
    assert abs(float(total) - float(want.sum())) <= total_bound(case.chunks) * float(want.sum())
    n2, t2 = _norms(case, edge["a"], edge["b32"], edge["dtype"], True)
    assert _same(n2, norms) and _same(t2, total)


def _unit_case(dtype, values):
    """One-element segments at stride 8 with a = values, b = 0: norms[k] = |values[k]|."""
    n = len(values)
    case = _Case([(8 * k, 1) for k in range(n)], 8 * n)
    a32 = np.zeros(8 * n, np.float32)
    a32[::8] = values
    return case, _t(P.rn16(a32, dtype), dtype), _t(np.zeros(8 * n, np.uint16), dtype)


@pytest.mark.parametrize("dtype,big,ones_first", [("bfloat16", 256.0, 320.0),
                                                  ("float16", 2048.0, 2112.0)])
def test_pure_total_is_the_in_order_16bit_sum(dtype, big, ones_first):
    """65 segments (more than a wave): one norm of 256 (2048 in fp16) followed
    by 64 ones keeps the total there — any tree or fp32 sum gives 320 (2112);
    the ones first do give 320 (2112)."""
    for vals, want in (([big] + [1.0] * 64, big), ([1.0] * 64 + [big], ones_first)):
        case, a, b = _unit_case(dtype, vals)
        norms, total = _norms(case, a, b, dtype, False)
        assert norms.cpu().tolist() == vals
        assert float(total) == want
        assert int(_bits(total)[0]) == P.running_total(P.rn16(norms.cpu().numpy(), dtype), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pure_global_memory_finish(dtype):
    """16,400 eight-element segments: 16,400 + 32,801 words do not fit the LDS
    finish.  Norms inside the restated interval, the total the in-order 16-bit
    running sum of the kernel's norms, a repeat the same bits."""
    nseg = 16400
    case = _Case([(8 * k, 8) for k in range(nseg)], 8 * nseg)
    assert not case.lds_finish
    ab, bb = P.inputs(8 * nseg, 5, dtype)
    a, b = _t(ab, dtype), _t(bb, dtype)
    norms, total = _norms(case, a, b, dtype, False)
    x = P.widen(P.diff16(ab, bb, dtype), dtype).reshape(nseg, 8)
    n64 = np.sqrt((x * x).sum(1))
    beta = P.norm_beta(8)
    lo = (n64 * (1 - beta)).astype(np.float32)
    lo = np.where(lo.astype(np.float64) > n64 * (1 - beta), np.nextafter(lo, np.float32(-np.inf)), lo)
    hi = (n64 * (1 + beta)).astype(np.float32)
    hi = np.where(hi.astype(np.float64) < n64 * (1 + beta), np.nextafter(hi, np.float32(np.inf)), hi)
    lo16, hi16 = P.rn16(lo, dtype), P.rn16(hi, dtype)
    assert (lo16 == hi16).mean() >= 0.9
    nb = P.rn16(norms.cpu().numpy(), dtype)
    assert np.array_equal(P.f32(nb, dtype), norms.cpu().numpy())
    assert ((lo16 <= nb) & (nb <= hi16)).all()
    assert int(_bits(total)[0]) == P.running_total(nb, dtype)
    n2, t2 = _norms(case, a, b, dtype, False)
    assert _same(n2, norms) and _same(t2, total)


# ------------------------------------------------------------ backward ----
@pytest.mark.parametrize("alpha", [1.0, -0.5])
def test_pure_gradient_bit_equal_to_torch_formula(edge, alpha):
    """grad_a bit-equal to rn16(rn16(gout * alpha) * rn16(d16 / norms[k])) by
    CPU torch from the kernel's own norms, zero where the norm is 0, grad_b its
    negation bit for bit, everything outside the segments the prior bits."""
    dtype, dt, case = edge["dtype"], edge["dt"], edge["case"]
    norms, _ = edge["pure"]
    gout = torch.tensor(0.7, device=DEV).to(dt)
    pa, pb = edge["prior"]["a"], edge["prior"]["b"]
    ga, gb = _grad(case, edge["a"], edge["b"], dtype, False, norms, gout, alpha, pa, pb)
    want = _torch_grad16(case, edge["a"], edge["b"], norms, gout, alpha, dt)
    inside = case.inside()
    assert np.array_equal(_bits(ga.cpu()[inside]), _bits(want[inside]))
    assert np.array_equal(_bits(gb.cpu()[inside]), P.neg16(_bits(ga.cpu()[inside])))
    assert _same(ga.cpu()[~inside], pa.cpu()[~inside]) and _same(gb.cpu()[~inside], pb.cpu()[~inside])
    o, m = case.segs[P.ZERO_SEG]
    assert not bool(ga[o:o + m].any()) and not bool(gb[o:o + m].any())
    ga2, gb2 = _grad(case, edge["a"], edge["b"], dtype, False, norms, gout, alpha, pa, pb)
    assert _same(ga2, ga) and _same(gb2, gb)


def test_mixed_gradient(edge):
    """grad_b (fp32) within prox.hip's 4u of gout * (a - b) / norms[k] in
    float64 with the kernel's own norms; grad_a == rn16(-grad_b) bit for bit;
    gaps untouched."""
    dtype, dt, case = edge["dtype"], edge["dt"], edge["case"]
    norms, _ = edge["mixed"]
    gout = torch.tensor(0.7, device=DEV)
    pa, pb = edge["prior"]["a"], edge["prior"]["b32"]
    ga, gb = _grad(case, edge["a"], edge["b32"], dtype, True, norms, gout, 1.0, pa, pb)
    assert gb.dtype == torch.float32 and ga.dtype == dt
    diff = edge["a"].cpu().double() - edge["b32"].cpu().double()
    d = torch.zeros(case.numel, dtype=torch.float64)
    for k, (o, m) in enumerate(case.segs):
        if m and float(norms[k]) != 0.0:
            d[o:o + m] = float(gout.cpu().double()) * diff[o:o + m] / norms[k].cpu().double()
    inside = case.inside()
    err = (gb.cpu().double() + d).abs()[inside]
    assert bool((err <= GRAD_BOUND * d.abs()[inside]).all()), float((err / d.abs()[inside].clamp_min(1e-300)).max() / U)
    assert np.array_equal(_bits(ga.cpu()[inside]), P.rn16((-gb).cpu().numpy()[inside.numpy()], dtype))
    assert _same(ga.cpu()[~inside], pa.cpu()[~inside]) and _same(gb.cpu()[~inside], pb.cpu()[~inside])


@pytest.mark.parametrize("with_gb", [True, False], ids=["gb", "gb_null"])
@pytest.mark.parametrize("flags", [0, 2, 4, 6, 1], ids=["none", "A", "B", "A|B", "ACC"])
@pytest.mark.parametrize("mixed", [False, True], ids=["pure", "mixed"])
def test_accumulate_flags_and_write_contract(edge, mixed, flags, with_gb):
    """Every accumulate flag, with grad_b given and NULL, over random prior
    contents: an accumulating 16-bit side is rn16(old + new) bit for bit (new:
    the overwrite launch's bits), an accumulating fp32 side old + new in one
    fp32 add; an overwritten side the overwrite launch's bits; the gaps — and
    all of B when grad_b is NULL — keep the prior bits."""
    from feddct_amd import _lib
    dtype, dt, case = edge["dtype"], edge["dt"], edge["case"]
    b = edge["b32"] if mixed else edge["b"]
    norms, _ = edge["mixed" if mixed else "pure"]
    gout = torch.tensor(-3.0, device=DEV).to(torch.float32 if mixed else dt)
    pa, pb = edge["prior"]["a"], edge["prior"]["b32" if mixed else "b"]
    na, nb_ = _grad(case, edge["a"], b, dtype, mixed, norms, gout, 1.0, pa, pb)   # overwrite
    ga, gb = _grad(case, edge["a"], b, dtype, mixed, norms, gout, 1.0, pa, pb, flags, with_gb)
    acc_a = bool(flags & (_lib.FA_PROX_ACCUMULATE | _lib.FA_PROX_ACCUMULATE_A))
    acc_b = bool(flags & (_lib.FA_PROX_ACCUMULATE | _lib.FA_PROX_ACCUMULATE_B))
    inside = case.inside()

    def acc(old, new):   # CPU torch: rn16(fp32(old) + fp32(new)), or the fp32 add
        return (old.cpu().float() + new.cpu().float()).to(old.dtype)

    want_a = acc(pa, na) if acc_a else na.cpu()
    assert _same(ga.cpu()[inside], want_a[inside]), "grad_a"
    assert _same(ga.cpu()[~inside], pa.cpu()[~inside]), "grad_a gap written"
    if with_gb:
        want_b = acc(pb, nb_) if acc_b else nb_.cpu()
        assert _same(gb.cpu()[inside], want_b[inside]), "grad_b"
        assert _same(gb.cpu()[~inside], pb.cpu()[~inside]), "grad_b gap written"
    else:
        assert _same(gb, pb), "grad_b written though NULL"


# ---------------------------------------------------- non-finite norms ----
def _small_case(dtype, poison):
    segs, numel = P.place([5, 8193, 1025, 4097])
    case = _Case(segs, numel)
    ab, bb = P.inputs(numel, 6, dtype)
    a, b = _t(ab, dtype), _t(bb, dtype)
    o = int(segs[1, 0])
    poison(a, b, o)
    norms, total = _norms(case, a, b, dtype, False)
    dt = TORCH_DT[dtype]
    gout = torch.tensor(0.7, device=DEV).to(dt)
    sent = torch.full((numel,), 7.0, device=DEV, dtype=dt)
    ga, gb = _grad(case, a, b, dtype, False, norms, gout, 1.0, sent, sent)
    want = _torch_grad16(case, a, b, norms, gout, 1.0, dt)
    rest = case.inside()
    rest[o:o + 8193] = False
    assert np.array_equal(_bits(ga.cpu()[rest]), _bits(want[rest])), "another tensor's gradient moved"
    return norms.cpu(), total.cpu(), ga.cpu()[o:o + 8193], gb.cpu()[o:o + 8193]


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_norm_gives_nans_for_its_tensor_only(dtype):
    def poison(a, b, o):
        a[o + 4100] = float("nan")
    norms, total, ga, gb = _small_case(dtype, poison)
    assert bool(norms[1].isnan()) and not bool(norms[[0, 2, 3]].isnan().any())
    assert bool(total.isnan())
    assert bool(ga.isnan().all()) and bool(gb.isnan().all())


def test_fp16_norm_overflowing_to_inf_gives_zero_gradients():
    """Differences of 60,000 in every chunk: the fp32 norm is finite, its fp16
    rounding +inf, and finite / inf gives zero gradients on both sides."""
    def poison(a, b, o):
        for i in (0, 1, 4100, 8192):
            a[o + i], b[o + i] = 60000.0, 0.0
    norms, total, ga, gb = _small_case("float16", poison)
    assert float(norms[1]) == float("inf") and float(total) == float("inf")
    assert not bool(ga.any()) and not bool(gb.any())


# ------------------------------------------------------------ refusals ----
def test_refusals_change_no_byte(edge):
    from feddct_amd import _lib
    L = _lib.lib
    dtype, dt, case = edge["dtype"], edge["dt"], edge["case"]
    el, F32 = _elem(dtype), _lib.FA_ELEM_F32
    other = _lib.FA_ELEM_F16 if el == _lib.FA_ELEM_BF16 else _lib.FA_ELEM_BF16
    a, b = edge["a"], edge["b"]
    norms, _ = edge["pure"]
    n_out = torch.full((case.nseg,), -1.0, device=DEV)
    t_out = torch.full((2,), -1.0, device=DEV)
    ga, gb = edge["prior"]["a"].clone(), edge["prior"]["b"].clone()
    gout = torch.tensor(0.7, device=DEV).to(dt)
    st = _stream()

    def norms_rc(plan, pa, ae, pb, be):
        return L.fa_prox_norms_elem(plan, pa, ae, pb, be, n_out.data_ptr(), t_out.data_ptr(), st)

    def grad_rc(plan, pa, ae, pb, be, pga=None, pgb=None, flags=0):
        return L.fa_prox_grad_elem(plan, pa, ae, pb, be, norms.data_ptr(), gout.data_ptr(), 1.0,
                                   pga or ga.data_ptr(), pgb or gb.data_ptr(), flags, st)

    h = case.plan.handle
    for ae, be in ((F32, el), (el, other), (other, el), (3, 3), (el, 5)):
        assert norms_rc(h, a.data_ptr(), ae, b.data_ptr(), be) == _lib.FA_E_INVAL, (ae, be)
        assert grad_rc(h, a.data_ptr(), ae, b.data_ptr(), be) == _lib.FA_E_INVAL, (ae, be)
    assert grad_rc(h, a.data_ptr(), el, b.data_ptr(), el, flags=8) == _lib.FA_E_INVAL
    # a segment at an offset of 4: legal for fp32, refused for a 16-bit bucket
    off4 = _Case([(0, 8), (12, 8)], 64)
    for be in (el, F32):
        assert norms_rc(off4.plan.handle, a.data_ptr(), el, b.data_ptr(), be) == _lib.FA_E_ALIGN
        assert grad_rc(off4.plan.handle, a.data_ptr(), el, b.data_ptr(), be) == _lib.FA_E_ALIGN
    # buckets 8 bytes off a 16-B boundary
    for i in range(4):
        p = [a.data_ptr(), b.data_ptr(), ga.data_ptr(), gb.data_ptr()]
        p[i] += 8
        assert grad_rc(h, p[0], el, p[1], el, p[2], p[3]) == _lib.FA_E_ALIGN, i
        if i < 2:
            assert norms_rc(h, p[0], el, p[1], el) == _lib.FA_E_ALIGN, i
    torch.cuda.synchronize()
    assert _same(n_out, torch.full_like(n_out, -1.0)) and _same(t_out, torch.full_like(t_out, -1.0))
    assert _same(ga, edge["prior"]["a"]) and _same(gb, edge["prior"]["b"])


def test_f32_pair_forwards_to_the_fp32_entry_points():
    """(F32, F32) — a plan with an offset of 4 included — gives fa_prox_norms /
    fa_prox_grad_ex's bits."""
    from feddct_amd import _lib
    L = _lib.lib
    case = _Case([(0, 9), (12, 4099)], 4120)
    g = torch.Generator(device=DEV).manual_seed(43)
    a = torch.randn(case.numel, device=DEV, generator=g)
    b = torch.randn(case.numel, device=DEV, generator=g)
    outs = []
    for elem in (False, True):
        norms, total = torch.zeros(2, device=DEV), torch.zeros((), device=DEV)
        ga, gb = torch.ones_like(a), torch.ones_like(a)
        gout = torch.tensor(0.7, device=DEV)
        F = (_lib.FA_ELEM_F32,)
        if elem:
            _lib.check(L.fa_prox_norms_elem(case.plan.handle, a.data_ptr(), *F, b.data_ptr(), *F,
                                            norms.data_ptr(), total.data_ptr(), _stream()))
            _lib.check(L.fa_prox_grad_elem(case.plan.handle, a.data_ptr(), *F, b.data_ptr(), *F,
                                           norms.data_ptr(), gout.data_ptr(), 0.5, ga.data_ptr(),
                                           gb.data_ptr(), 2, _stream()))
        else:
            _lib.check(L.fa_prox_norms(case.plan.handle, a.data_ptr(), b.data_ptr(),
                                       norms.data_ptr(), total.data_ptr(), _stream()))
            _lib.check(L.fa_prox_grad_ex(case.plan.handle, a.data_ptr(), b.data_ptr(),
                                         norms.data_ptr(), gout.data_ptr(), 0.5, ga.data_ptr(),
                                         gb.data_ptr(), 2, _stream()))
        torch.cuda.synchronize()
        outs.append((norms, total, ga, gb))
    for x, y in zip(*outs):
        assert _same(x, y)
