"""dlrm.MLP(return_hidden_layer_feature=True) (tzrec/modules/mlp.py:166-177): forward returns {"hidden_layer<i>": layer i's
output, "hidden_layer_end": the last one's}, the layers one at a time -- through the fused Linear+ReLU call where the MLP is plain
and on the device, through the module list otherwise -- and every default call is what it was."""
import pytest
import torch
from torch import nn

from torcheasyrec_amd.dlrm import MLP

KWARGS = {"plain": {}, "bn": {"use_bn": True}, "ln": {"use_ln": True}, "dropout": {"dropout_ratio": [0.5]}, "gelu_no_bias": {"activation": "nn.GELU", "bias": False},
          "no_activation": {"activation": ""}}


def by_layer(mlp, x):
    """the perceptrons one after the other, in plain torch: Linear, then everything up to the next Linear"""
    outs = []
    for m in mlp.mlp:
        if isinstance(m, nn.Linear):
            outs.append(None)
        x = m(x)
        outs[-1] = x
    return outs


@pytest.mark.parametrize("kind", sorted(KWARGS))
@pytest.mark.parametrize("hidden", [[12], [32, 16, 8]])
def test_the_dict_holds_every_layers_output(dev, kind, hidden):
    torch.manual_seed(0)
    mlp = MLP(20, hidden, return_hidden_layer_feature=True, **KWARGS[kind]).to(dev).eval()  # (eval: dropout and batch norm repeatable)
    assert mlp._plain == (kind == "plain")
    x = torch.randn(9, 20, device=dev)
    out = mlp(x)
    assert list(out) == [f"hidden_layer{i}" for i in range(len(hidden))] + ["hidden_layer_end"]
    want = by_layer(mlp, x)
    assert len(want) == len(hidden)
    for i, w in enumerate(want):
        assert out[f"hidden_layer{i}"].shape == (9, hidden[i])
        torch.testing.assert_close(out[f"hidden_layer{i}"], w, rtol=1e-5, atol=1e-6)  # (the fused GEMM epilogue against Linear + ReLU)
    assert out["hidden_layer_end"] is out[f"hidden_layer{len(hidden) - 1}"]


@pytest.mark.parametrize("kind", sorted(KWARGS))
def test_the_default_returns_the_tensor_it_did(dev, kind):
    torch.manual_seed(1)
    a = MLP(20, [16, 8], **KWARGS[kind]).to(dev).eval()
    b = MLP(20, [16, 8], return_hidden_layer_feature=True, **KWARGS[kind]).to(dev).eval()
    b.load_state_dict(a.state_dict())  # the same parameter names either way
    assert not a.return_hidden_layer_feature and list(a.state_dict()) == list(b.state_dict())
    x = torch.randn(9, 20, device=dev)
    y = a(x)
    assert isinstance(y, torch.Tensor) and y.shape == (9, 8)
    torch.testing.assert_close(y, a.mlp(x), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(y, b(x)["hidden_layer_end"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("kind", ["plain", "ln"])
def test_gradients_flow_from_a_hidden_entry_and_the_end_together(dev, kind):
    torch.manual_seed(2)
    mlp = MLP(20, [16, 8], return_hidden_layer_feature=True, **KWARGS[kind]).to(dev)
    twin = MLP(20, [16, 8], **KWARGS[kind]).to(dev)
    twin.load_state_dict(mlp.state_dict())
    x = torch.randn(9, 20, device=dev)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    out = mlp(xa)
    (out["hidden_layer0"].square().sum() * 0.5 + out["hidden_layer_end"].sum() * 1.5).backward()
    hs = by_layer(twin, xb)
    (hs[0].square().sum() * 0.5 + hs[1].sum() * 1.5).backward()
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-4, atol=1e-5)
    for (n, p), (_, q) in zip(mlp.named_parameters(), twin.named_parameters()):
        assert p.grad is not None and float(p.grad.abs().max()) > 0, n
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-4, atol=1e-5, msg=lambda m, n=n: f"{n}: {m}")
