"""The references of tests/eca_ref.py against torch itself: the closed-form backward of the ECA residual unit equals autograd in
fp64, the window size rule gives the sizes of the four ResNet stages, and the restated module is the Conv1d it says it is."""
import pytest
import torch

import eca_ref as E


def test_kernel_size_rule():
    assert [E.eca_k(c) for c in (64, 256, 512, 1024, 2048)] == [3, 5, 5, 5, 7]
    assert all(E.eca_k(c) % 2 == 1 and E.eca_k(c) >= 3 for c in (8, 16, 24, 96, 4096))


@pytest.mark.parametrize('n,hw,c,k', [(1, 1, 8, 3), (3, 5, 24, 5), (2, 16, 8, 7), (2, 49, 64, 9)])
def test_closed_form_backward_equals_autograd(n, hw, c, k):
    g = torch.Generator().manual_seed(n * 1000 + hw * 10 + k)
    z = torch.randn(n, hw, c, generator=g, dtype=torch.float64, requires_grad=True)
    sc = torch.randn(n, hw, c, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(k, generator=g, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(n, hw, c, generator=g, dtype=torch.float64)
    out, mean, gate = E.eca_residual_ref(z, sc, w)
    out.backward(dout)
    r = E.eca_residual_bwd_ref(dout, out.detach(), z.detach(), w.detach(), mean.detach(), gate.detach())
    for name, got, want in (('dz', r['dz'], z.grad), ('dshort', r['dshort'], sc.grad), ('dw', r['dw'], w.grad)):
        assert torch.allclose(got, want, rtol=1e-11, atol=1e-12), (name, float((got - want).abs().max()))


def test_module_is_the_unit():
    """EcaModule (the network's restatement) followed by add + ReLU is eca_residual_ref"""
    torch.manual_seed(0)
    m = E.EcaModule(64).double()
    x, sc = torch.randn(2, 64, 5, 3, dtype=torch.float64), torch.randn(2, 64, 5, 3, dtype=torch.float64)
    want = torch.relu(m(x) + sc)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(2, 15, 64)      # noqa: E731
    got, _, _ = E.eca_residual_ref(rows(x), rows(sc), m.conv.weight.detach().view(-1))
    assert m.conv.weight.shape == (1, 1, 3)
    assert torch.allclose(got, rows(want), rtol=1e-12, atol=1e-13)
