"""feddct_amd.prox.proximal_term for fp16 / bf16 models: a 16-bit client with
a 16-bit global (pure), with an fp32 master global (mixed), and the all-fp32
pair (nothing moved), against the reference's loop on CPU twins — the term's
and every gradient's dtype, the value, every gradient element within the
budget of its roundings; the one-node form accumulating; a server_aggregate
round between two steps keeping the arenas; and the pairs that still refuse."""
import copy

import numpy as np
import pytest
import torch

import prox16ref as P
from test_gpu_prox_edges import GRAD_BOUND, norm_bound, total_bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TORCH_DT = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}
NAME = {v: k for k, v in TORCH_DT.items()}
FORMS = [("bfloat16", "bfloat16"), ("float16", "float16"), ("bfloat16", "float32"),
         ("float16", "float32"), ("float32", "float32")]
IDS = ["pure_bf16", "pure_fp16", "mixed_bf16", "mixed_fp16", "fp32"]


class Net(torch.nn.Module):
    """Parameters of 1, 7, 8, 100 and 4,097 elements (the vector edge, more
    than one chunk) and a BatchNorm: 16-bit buffers and an int64 key."""

    def __init__(self):
        super().__init__()
        self.p1 = torch.nn.Parameter(torch.randn(1))
        self.p7 = torch.nn.Parameter(torch.randn(7))
        self.p8 = torch.nn.Parameter(torch.randn(8))
        self.big = torch.nn.Parameter(torch.randn(4097))
        self.lin = torch.nn.Linear(10, 10, bias=False)
        self.bn = torch.nn.BatchNorm1d(4)


def _pair(cdt, gdt, seed):
    """(client, global) on the GPU, the client's parameters the global's plus
    0.05 randn, and their CPU twins made before anything is bound."""
    torch.manual_seed(seed)
    g = Net()
    c = copy.deepcopy(g)
    with torch.no_grad():
        for p in c.parameters():
            p.add_(0.05 * torch.randn_like(p))
    c, g = c.to(TORCH_DT[cdt]), g.to(TORCH_DT[gdt])
    tc, tg = copy.deepcopy(c), copy.deepcopy(g)
    return c.to(DEV), g.to(DEV), tc, tg


def _loop(c, g):
    proximal_term = 0.0
    for w, w_t in zip(c.parameters(), g.parameters()):
        proximal_term += (w - w_t).norm(2)
    return proximal_term


def _check_step(c, g, tc, tg, cdt, gdt, flat):
    """One forward and backward of both, compared."""
    from feddct_amd.prox import proximal_term
    ref = _loop(tc, tg)
    (ref * 0.37).backward()
    got = proximal_term(c, g, flat_grads=flat)
    (got * 0.37).backward()
    torch.cuda.synchronize()
    assert got.dtype == ref.dtype and got.dim() == 0
    got, ref = got.detach(), ref.detach()
    pure = gdt != "float32"
    K = len(list(tc.parameters()))
    chunks = [-(-p.numel() // P.CHUNK) for p in tc.parameters()]
    with torch.no_grad():
        d = [(w - w_t).double() for w, w_t in zip(tc.parameters(), tg.parameters())]
    n64 = [float(x.norm(2)) for x in d]
    if pure:
        # each 16-bit norm is within u16 + beta of n64 on either side, and the
        # K - 1 adds of the running sum round once each
        beta = max(P.norm_beta(p.numel()) for p in tc.parameters())
        lim = (2 * (P.U16[cdt] + beta) + 2 * (K - 1) * P.U16[cdt]) * sum(n64)
        print(f"term: got {float(got)!r} ref {float(ref)!r} bit-equal {float(got) == float(ref)}")
        assert abs(float(got) - float(ref)) <= lim
        scale = float(torch.tensor(0.37).to(TORCH_DT[cdt]))   # gout16
    else:
        assert abs(float(got) - sum(n64)) <= total_bound(chunks) * sum(n64)
        scale = float(np.float32(0.37))
    for side, model, twin, sign in (("client", c, tc, 1.0), ("global", g, tg, -1.0)):
        for (name, p), q, x, n, ch in zip(model.named_parameters(), twin.parameters(), d, n64,
                                          chunks):
            assert p.grad is not None and p.grad.dtype == q.grad.dtype == p.dtype, (side, name)
            want = sign * scale * x / n
            got_g = p.grad.detach().cpu().double()
            if p.dtype == torch.float32:
                lim = (GRAD_BOUND + norm_bound(ch)) * want.abs()
            else:
                lim = torch.from_numpy(P.grad_limit(want.numpy(), NAME[p.dtype]))
                own = ((q.grad.double() - want).abs() / lim).max()
                print(f"{side} {name}: torch's own CPU result at {float(own):.2f} of the limit")
            err = (got_g - want).abs()
            print(f"{side} {name}: worst {float((err / lim).max()):.2f} of the limit")
            assert bool((err <= lim).all()), (side, name)


@pytest.mark.parametrize("cdt,gdt", FORMS, ids=IDS)
def test_value_and_gradients_against_the_reference_loop(cdt, gdt):
    c, g, tc, tg = _pair(cdt, gdt, 51)
    _check_step(c, g, tc, tg, cdt, gdt, flat=False)


@pytest.mark.parametrize("cdt,gdt", FORMS[:4], ids=IDS[:4])
def test_flat_grads_accumulates_in_each_sides_dtype(cdt, gdt):
    """The one-node form (the Python node for 16-bit pairs): the first
    backward meets the budget, the .grad are views of one bucket per side in
    that side's dtype, and a second backward accumulates: rn16(old + new) for
    a 16-bit side, one fp32 add for an fp32 one — bit for bit."""
    from feddct_amd.prox import proximal_term
    c, g, tc, tg = _pair(cdt, gdt, 52)
    _check_step(c, g, tc, tg, cdt, gdt, flat=True)
    first = [p.grad.detach().clone() for m in (c, g) for p in m.parameters()]
    (proximal_term(c, g, flat_grads=True) * 0.37).backward()
    torch.cuda.synchronize()
    for p, old in zip([p for m in (c, g) for p in m.parameters()], first):
        want = (old.float() + old.float()).to(old.dtype)
        iv = torch.int16 if old.element_size() == 2 else torch.int32
        assert p.grad.dtype == p.dtype
        assert torch.equal(p.grad.view(iv), want.view(iv))


@pytest.mark.parametrize("cdt,gdt", [FORMS[0], FORMS[3]], ids=[IDS[0], IDS[3]])
def test_a_round_between_two_steps_keeps_the_arenas(cdt, gdt):
    """proximal_term binds the arenas server_aggregate binds: a round between
    two steps leaves them in place and the cached term valid."""
    from feddct_amd import server_aggregate
    from feddct_amd.prox import proximal_term
    c, g, _, _ = _pair(cdt, gdt, 53)
    c2 = copy.deepcopy(c)
    (proximal_term(c, g) * 0.37).backward()
    term = c.__dict__["_fa_prox"][id(g)]
    arenas = (c._fa_arena, g._fa_arena)
    server_aggregate(g, [c, c2])
    torch.cuda.synchronize()
    assert c._fa_arena is arenas[0] and g._fa_arena is arenas[1]
    assert term.valid()
    t = proximal_term(c, g)
    assert c.__dict__["_fa_prox"][id(g)] is term
    t.backward()
    torch.cuda.synchronize()
    # after the broadcast the client holds the global's values (rounded to its dtype)
    assert bool(torch.isfinite(t)) and t.dtype == (TORCH_DT[cdt] if gdt != "float32"
                                                   else torch.float32)
    server_aggregate(g, [c, c2])
    assert c._fa_arena is arenas[0] and g._fa_arena is arenas[1] and term.valid()


def test_pairs_that_still_refuse():
    import feddct_amd
    from feddct_amd.prox import ProximalTerm
    torch.manual_seed(54)
    # a 16-bit global over fp32 clients
    with pytest.raises(NotImplementedError, match="supported pairs"):
        ProximalTerm(Net().to(DEV), Net().half().to(DEV))
    # mixed dtypes inside one model
    c = Net().bfloat16()
    c.big.data = c.big.data.float()
    with pytest.raises(NotImplementedError, match="supported pairs"):
        ProximalTerm(c.to(DEV), Net().bfloat16().to(DEV))
    # clients of one 16-bit dtype against a global of the other
    with pytest.raises(NotImplementedError, match="supported pairs"):
        ProximalTerm(Net().half().to(DEV), Net().bfloat16().to(DEV))
    # host-resident 16-bit models
    with pytest.raises(NotImplementedError, match="supported pairs"):
        ProximalTerm(Net().half(), Net().half())
    # the torch_gpu order, whose 16-bit rounds are staged
    feddct_amd.set_summation_order("torch_gpu")
    try:
        with pytest.raises(NotImplementedError, match="supported pairs"):
            ProximalTerm(Net().half().to(DEV), Net().half().to(DEV))
    finally:
        feddct_amd.set_summation_order("torch_cpu")
