"""GPU tests of gst_reg_quad_fwd / gst_reg_quad_bwd (libgslora_train.so): sum_i omega_i (p_i - p0_i)^2 and its gradient, the arithmetic of the
reference's get_reg_loss (engine_cl.py:455-457). Lengths around the lane, wave and chunk edges of the kernels (1, 63, 64, 65, 4097) and a
whole FFN weight of the flagship model plus a ragged tail (65 920); with an importance tensor and without (the L2 baseline).
Forward: against float64 within n * 2^-24 * sum |terms| (an f32 sum of n correctly rounded terms in any order). Backward: bit-equal to the f32 expression
((coef * 2) * omega) * (p - p0) added to a banded g."""
import pytest
import torch

from guard_bands import Banded

pytestmark = pytest.mark.gpu

LENGTHS = [1, 63, 64, 65, 4097, 65920]


def LT():
    from gslora_hip import _lib_train
    return _lib_train


def tensors(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g), torch.randn(n, generator=g), torch.rand(n, generator=g) * 3.0


@pytest.mark.parametrize("with_omega", [False, True], ids=["l2", "omega"])
@pytest.mark.parametrize("n", LENGTHS)
def test_forward_matches_float64(n, with_omega):
    lt = LT()
    pv, p0v, omv = tensors(n, n)
    p, p0 = Banded((n,), torch.float32, pv), Banded((n,), torch.float32, p0v)
    om = Banded((n,), torch.float32, omv) if with_omega else None
    out = Banded((1,), torch.float32)
    ws = Banded((lt.load().gst_reg_quad_ws_elems(n),), torch.float32)
    lt.reg_quad_fwd(p.view, p0.view, om.view if om else None, out.view, ws=ws.view)
    torch.cuda.synchronize()
    assert p.bands_intact() and p0.bands_intact() and (om is None or om.bands_intact()) and out.bands_intact() and ws.bands_intact()
    terms = (omv.double() if with_omega else 1.0) * (pv.double() - p0v.double()) ** 2
    want, bound = terms.sum().item(), n * 2.0 ** -24 * terms.abs().sum().item()
    got = out.view.item()
    print(f"reg_quad_fwd n={n} omega={with_omega}: |err| / bound = {abs(got - want) / bound:.4f}")
    assert abs(got - want) <= bound
    # accumulate = 1 adds to what out holds; the same call again gives the same bits
    first = out.view.clone()
    lt.reg_quad_fwd(p.view, p0.view, om.view if om else None, out.view, accumulate=True, ws=ws.view)
    assert torch.equal(out.view, first + first)
    lt.reg_quad_fwd(p.view, p0.view, om.view if om else None, out.view, ws=ws.view)
    assert torch.equal(out.view, first)


@pytest.mark.parametrize("with_omega", [False, True], ids=["l2", "omega"])
@pytest.mark.parametrize("n", LENGTHS)
def test_backward_is_the_f32_expression_bit_for_bit(n, with_omega):
    lt = LT()
    pv, p0v, omv = tensors(n, 100 + n)
    gv = torch.randn(n, generator=torch.Generator().manual_seed(n))
    p, p0 = Banded((n,), torch.float32, pv), Banded((n,), torch.float32, p0v)
    om = Banded((n,), torch.float32, omv) if with_omega else None
    g = Banded((n,), torch.float32, gv)
    coef = Banded((1,), torch.float32, torch.tensor([0.37]))
    lt.reg_quad_bwd(p.view, p0.view, om.view if om else None, coef.view, g.view)
    torch.cuda.synchronize()
    assert p.bands_intact() and p0.bands_intact() and (om is None or om.bands_intact()) and coef.bands_intact() and g.outside_intact()
    c = torch.tensor(0.37) * 2.0
    want = gv + (c * omv if with_omega else c) * (pv - p0v)      # f32 on the CPU: every product and the sum rounded on its own
    assert torch.equal(g.view.cpu(), want)


def test_refusals():
    lib = LT().load()
    p = 4096
    assert lib.gst_reg_quad_fwd(p, p, None, 0, p, 0, p, None) == -1 and b"n >= 1" in lib.gst_last_error()
    assert lib.gst_reg_quad_fwd(p, p, None, 5, p, 0, None, None) == -1 and b"null ws" in lib.gst_last_error()
    assert lib.gst_reg_quad_bwd(p, p, None, 5, None, p, None) == -1 and b"gst_reg_quad_bwd" in lib.gst_last_error()
    assert lib.gst_reg_quad_ws_elems(0) == -1
