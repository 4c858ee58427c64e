"""GPU tests of libgslora_reg.so, the kernels alone: gsr_importance_acc (bit-equal to the torch expressions of the reference's importance
loops on the CPU, at every relative alignment of its two pointers, with the overflow guard), gsr_sq_mean_fwd / _bwd (MAS's objective: the
forward against float64 within the bound of its own reduction tree, the backward bit-equal to torch autograd on the CPU) and the batched
quadratic regulariser gsr_reg_multi_* (bit-equal, value and gradients, to step.reg_loss — the sequence of gst_reg_quad_* launches)."""
import math

import pytest
import torch

from guard_bands import Banded

pytestmark = pytest.mark.gpu

PAD = 1024      # elements in front of and behind a misaligned placement (a multiple of 4: the offset alone decides the alignment)
SPECIAL = [0.0, -0.0, -1.5, 1e-30, -1e-30, 1e-20, -1e-20, 1e19, -1e19, 3.0]


def LR():
    from gslora_hip import _lib_reg
    return _lib_reg


class Placed:
    """n f32 values at `off` elements behind a 16-byte boundary, NaN all around."""

    def __init__(self, values, off):
        n = values.numel()
        self.buf = torch.full((2 * PAD + n + 4,), float("nan"), device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.hi = PAD + off, PAD + off + n
        self.view = self.buf[self.lo:self.hi]
        self.view.copy_(values)
        self.before = self.buf.view(torch.int32).clone()
        assert self.view.data_ptr() % 16 == 4 * off

    def outside_intact(self):
        now = self.buf.view(torch.int32)
        return torch.equal(now[:self.lo], self.before[:self.lo]) and torch.equal(now[self.hi:], self.before[self.hi:])

    def untouched(self):
        return torch.equal(self.buf.view(torch.int32), self.before)


def importance_inputs(n):
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen) * 10.0
    k = min(n, len(SPECIAL))
    idx = torch.arange(k) * max(1, n // len(SPECIAL))      # spread over the tensor: head, vector body and tail all meet some
    g[idx] = torch.tensor(SPECIAL[:k])
    return torch.rand(n, generator=gen) * 2.0, g


def torch_importance(omega, g, kind, a, b):
    p = omega.clone()
    if kind == 0:
        p += g ** 2 * a / b      # reference train/train_own_forget_cl.py:1505-1509 (a = len(samples), b = len(subdataloader): Python ints)
    else:
        p += g.abs() / b         # :1556-1558
    return p


@pytest.mark.parametrize("kind", [0, 1], ids=["ewc", "mas"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 1025, 2 ** 20 + 3])
def test_importance_acc_is_the_torch_expression_bit_for_bit(n, kind):
    lr = LR()
    omega, g = importance_inputs(n)
    want = torch_importance(omega, g, kind, 3, 7)
    assert torch.isfinite(want).all()
    if n >= 255 and kind == 0:      # the inputs hold what they claim: a square that underflows to zero and one that is subnormal
        sq = (g ** 2)
        assert ((sq == 0) & (g != 0)).any() and ((sq > 0) & (sq < 1.1754944e-38)).any()
    for off_o in range(4):
        for off_g in range(4):
            po, pg = Placed(omega, off_o), Placed(g, off_g)
            lr.importance_acc(po.view, pg.view, kind, 3, 7)
            torch.cuda.synchronize()
            got = po.view.cpu()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (off_o, off_g, int((got != want).sum()))
            assert po.outside_intact() and pg.untouched(), (off_o, off_g)


@pytest.mark.parametrize("kind", [0, 1], ids=["ewc", "mas"])
def test_importance_acc_guard_skips_a_saturated_backward(kind):
    lr = LR()
    n = 1025
    omega, g = importance_inputs(n)
    want = torch_importance(omega, g, kind, 3, 7)
    skipped = torch.zeros(1, device="cuda", dtype=torch.int32)
    expect = 0
    for value, applied in ((65503.0, True), (65504.0, False), (float("inf"), False), (float("nan"), False), (None, True)):
        po, pg = Placed(omega, 1), Placed(g, 1)
        guard = None if value is None else torch.tensor([value], device="cuda")
        lr.importance_acc(po.view, pg.view, kind, 3, 7, guard, skipped)
        torch.cuda.synchronize()
        if applied:
            assert torch.equal(po.view.cpu().view(torch.int32), want.view(torch.int32)), value
        else:
            expect += 1
            assert po.untouched(), value
        assert pg.untouched() and skipped.item() == expect, value
    po, pg = Placed(omega, 0), Placed(g, 0)      # the counter is optional
    lr.importance_acc(po.view, pg.view, kind, 3, 7, torch.tensor([float("inf")], device="cuda"), None)
    torch.cuda.synchronize()
    assert po.untouched()


# ---------------------------------------------------------------------------------------------------------------- mean of squares
def sq_mean_roundings(n):
    """f32 roundings on the longest path of gsr_sq_mean_fwd (csrc/reg.hip): the thread's f64 sum rounded once; block_sum = 6 wave steps + 3
    adds over the four waves (0 + sm[0] is exact); the reduce kernel's strided sum (at most ceil(nblk / 256) adds), its block_sum, the
    division."""
    nblk = min(1024, -(-n // 1024))
    return 1 + (6 + 3) + -(-nblk // 256) + (6 + 3) + 1


@pytest.mark.parametrize("pad", [0, 3], ids=["ld=C", "ld=C+3"])
@pytest.mark.parametrize("B,C", [(1, 1), (2, 12), (3, 1025), (37, 100)])
def test_sq_mean_forward_and_backward(B, C, pad):
    lr = LR()
    xv = torch.randn(B, C, generator=torch.Generator().manual_seed(B * 1000 + C)) * 3.0
    x = Banded((B, C), torch.float32, xv, ld=C + pad)
    out, ws = Banded((1,), torch.float32), Banded((lr.sq_mean_ws_elems(B, C),), torch.float32)
    lr.sq_mean_fwd(x.view, out.view, ws.view)
    torch.cuda.synchronize()
    assert x.bands_intact() and out.bands_intact() and ws.bands_intact()
    n = B * C
    want = (xv.double() ** 2).sum().item() / n
    bound = ((1.0 + 2.0 ** -24) ** sq_mean_roundings(n) - 1.0 + n * 2.0 ** -53) * want      # every addend is >= 0: the bound is relative
    got = out.view.item()
    print(f"sq_mean_fwd B={B} C={C} ld=C+{pad}: |err| / bound = {abs(got - want) / bound:.4f}")
    assert abs(got - want) <= bound
    first = out.view.clone()
    lr.sq_mean_fwd(x.view, out.view, ws.view)
    assert torch.equal(out.view, first)      # the same bits on every call
    for gout in (1.0, 0.37):
        xc = xv.clone().requires_grad_(True)
        xc.pow(2).mean().backward(torch.tensor(gout))
        dx = Banded((B, C), torch.float32, ld=C + pad)
        gdev = Banded((1,), torch.float32, torch.tensor([gout]))
        lr.sq_mean_bwd(x.view, gdev.view, dx.view)
        torch.cuda.synchronize()
        assert dx.bands_intact() and x.bands_intact() and gdev.bands_intact() and dx.unwritten() == 0      # the pad columns keep the sentinel
        assert torch.equal(dx.view.cpu().view(torch.int32), xc.grad.view(torch.int32)), gout


def test_sq_mean_autograd_node_matches_torch():
    from gslora_hip import reg
    xv = torch.randn(5, 33, generator=torch.Generator().manual_seed(5))
    x = xv.cuda().requires_grad_(True)
    (reg.sq_mean(x) * 0.37).backward()
    xc = xv.clone().requires_grad_(True)
    (xc.pow(2).mean() * 0.37).backward()
    assert torch.equal(x.grad.cpu(), xc.grad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reg.sq_mean(xv)


# ---------------------------------------------------------------------------------------------------------------- batched regulariser
def on_gpu(values, off=None):
    """values on the GPU: its own allocation, or (off given) a view `off` floats behind a 16-byte boundary of a larger one."""
    if off is None:
        return values.cuda()
    buf = torch.zeros(values.numel() + 8, device="cuda")
    view = buf[4 + off:4 + off + values.numel()].view(values.shape)
    view.copy_(values)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * off and view.is_contiguous()
    return view


class Bag(torch.nn.Module):
    """offsets: per tensor, how many floats behind a 16-byte boundary it starts (None: every parameter is its own allocation)."""

    def __init__(self, sizes, seed, offsets=None):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.offsets = dict(zip((f"w.{i}" for i in range(len(sizes))), offsets or [None] * len(sizes)))
        self.w = torch.nn.ParameterList([torch.nn.Parameter(on_gpu(torch.randn(n, generator=g), off) if off is not None else torch.randn(n, generator=g))
                                         for n, off in zip(sizes, self.offsets.values())])


def make_terms(model, n_terms, seed):
    """importance and task_param sit where their parameter sits relative to a 16-byte boundary (Bag.offsets)."""
    g = torch.Generator().manual_seed(seed)
    terms = {}
    for k in range(n_terms):
        terms[k] = {"importance": {n: (None if (n_terms > 1 and k == 1) else on_gpu(torch.rand(p.shape, generator=g) * 3.0, model.offsets[n]))
                                   for n, p in model.named_parameters()},
                    "task_param": {n: on_gpu(p.detach().cpu() + 0.1 * torch.randn(p.shape, generator=g), model.offsets[n])
                                   for n, p in model.named_parameters()}}
    return terms


# misaligned: no tensor of an entry is 16-byte aligned, so gsr_reg_multi_bwd walks every chunk element by element (its scalar branch; 4099
# elements are five chunks with an odd tail); step.reg_loss's gst_reg_quad_bwd has no vector branch at all
@pytest.mark.parametrize("sizes,n_terms,offsets", [((1,), 1, None), ((1, 1023, 1024, 1025, 2 ** 20 + 5), 3, None), ((5, 1025, 4099), 3, (1, 2, 3))],
                         ids=["one-element", "five-tensors-three-terms", "misaligned"])
def test_batched_regulariser_is_reg_loss_bit_for_bit(sizes, n_terms, offsets):
    from gslora_hip import reg, step
    lam = 0.37
    a, b = Bag(sizes, 1, offsets).cuda(), Bag(sizes, 1, offsets).cuda()
    for m in (a, b):
        assert all(p.data_ptr() % 16 == 4 * (off or 0) for p, off in zip(m.parameters(), m.offsets.values()))
    terms = make_terms(a, n_terms, 2)
    rt = reg.RegTerms(b, terms, lam)
    for rnd in range(2):      # the second round accumulates into the non-zero gradients of the first
        want = step.reg_loss(a, terms, lam, torch.device("cuda"))
        got = rt.loss()
        assert got.dim() == 0 and torch.equal(got.detach().view(torch.int32), want.detach().view(torch.int32)), (got.item(), want.item())
        (want * 1.7).backward()
        (got * 1.7).backward()
        for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            assert q.grad.shape == p.grad.shape and torch.equal(q.grad.view(torch.int32), p.grad.view(torch.int32)), (rnd, n)
    # ... and within the float64 bound of tests/test_hip_reg_quad.py: n * 2^-24 * sum |terms| per entry, one more rounding per entry added
    # to the running total, one for the product with lambda
    tot, bound = 0.0, 0.0
    for t in terms.values():
        for n, p in a.named_parameters():
            om = t["importance"][n]
            e = ((1.0 if om is None else om.double()) * (p.detach().double() - t["task_param"][n].double()) ** 2).sum().item()
            tot += e
            bound += p.numel() * 2.0 ** -24 * e
    bound = lam * (bound + (n_terms * len(sizes) + 1) * 2.0 ** -24 * tot)
    print(f"reg_multi {len(sizes)} tensors x {n_terms} terms: |err| / bound = {abs(got.item() - lam * tot) / bound:.4f}")
    assert abs(got.item() - lam * tot) <= bound
    assert rt.rebuilds == 0


def test_the_table_is_rebuilt_when_a_parameter_moves():
    from gslora_hip import reg, step
    sizes = (7, 1025)
    a, b = Bag(sizes, 3).cuda(), Bag(sizes, 3).cuda()
    terms = make_terms(a, 2, 4)
    rt = reg.RegTerms(b, terms, 2.0)
    first = rt.loss().detach().clone()
    fresh = torch.randn(1025, generator=torch.Generator().manual_seed(9)).cuda()
    old = b.w[1].data      # (kept alive: the allocator must not hand the same address back)
    a.w[1].data.copy_(fresh)
    b.w[1].data = fresh.clone()
    assert b.w[1].data_ptr() != old.data_ptr()
    want = step.reg_loss(a, terms, 2.0, torch.device("cuda"))
    got = rt.loss()
    assert rt.rebuilds == 1 and torch.equal(got.detach(), want.detach()) and not torch.equal(got.detach(), first)
    got.backward()
    want.backward()
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p.grad, q.grad)
    assert rt.loss() is not None and rt.rebuilds == 1


def test_reg_terms_validates_like_reg_loss():
    from gslora_hip import reg
    b = Bag((4, 5), 1).cuda()
    terms = make_terms(b, 1, 1)
    terms[0]["task_param"]["w.1"] = torch.zeros(6).cuda()
    with pytest.raises(ValueError, match="importance / task_param of 'w.1' do not have the parameter's shape"):
        reg.RegTerms(b, terms, 1.0)
    with pytest.raises(RuntimeError, match="must be a contiguous f32 tensor on the GPU"):
        reg.RegTerms(Bag((4,), 1), make_terms(Bag((4,), 1), 1, 1), 1.0)
    assert math.isfinite(reg.RegTerms(b, make_terms(b, 1, 1), 1.0).loss().item())
