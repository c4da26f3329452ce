"""Window attention on the composed (CPU, fp32) route against the float64
reference of _winref.py, and the Swin wiring (no GPU)."""

import pytest
import torch

import _winref as wr
from pytorch_ddp_template_amd.models import build_model, swin_tiny
from pytorch_ddp_template_amd.ops import CrossEntropyLoss, window_attention
from pytorch_ddp_template_amd.optim import param_groups_no_decay


@pytest.mark.parametrize("n,h,w,heads,shift", [(2, 14, 14, 3, 3),
                                               (1, 14, 21, 2, 0)])
def test_composed_route_matches_float64(n, h, w, heads, shift):
    qkv, table, dout = wr.inputs(n, h, w, heads)
    scale = 32 ** -0.5
    ref = wr.win_attn_ref(qkv, table, heads, shift, scale, dout)
    qkv.requires_grad_(True)
    table.requires_grad_(True)
    out = window_attention(qkv, table, heads, shift, scale)
    out.backward(dout)
    for got, want in zip((out, qkv.grad, table.grad), ref):
        assert torch.allclose(got.detach().double(), want, rtol=1e-4, atol=1e-5)


def test_swin_tiny_parameter_count():
    m = swin_tiny(1000)
    assert sum(p.numel() for p in m.parameters()) == 28_288_354
    skip = m.no_weight_decay()
    assert len(skip) == 12 and all(
        n.endswith("attn.relative_position_bias_table") for n in skip)
    decay = param_groups_no_decay(m, 0.05)[0]["params"]
    assert all(p.shape != (169, h) for p in decay for h in (3, 6, 12, 24))
    # the 7x7 stage is one window: never shifted
    assert [b.attn.shift for s in m.stages for b in s] == \
        [0, 3, 0, 3, 0, 3, 0, 3, 0, 3, 0, 0]


def test_tiny_swin_runs_and_keys_do_not_depend_on_drop_path():
    m = wr.tiny_swin(drop_path=0.2)
    assert list(m.state_dict()) == list(wr.tiny_swin().state_dict())
    x = torch.randn(2, 28, 28, 3)
    loss = CrossEntropyLoss()(m(x), torch.tensor([1, 7]))
    loss.backward()
    assert torch.isfinite(loss)
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in m.parameters())


def test_errors():
    table = torch.zeros(169, 2)
    with pytest.raises(ValueError, match="head dim"):
        window_attention(torch.zeros(1, 7, 7, 3 * 2 * 16), table, 2, 0, 1.0)
    with pytest.raises(ValueError, match="multiples of the window"):
        window_attention(torch.zeros(1, 15, 14, 3 * 2 * 32), table, 2, 0, 1.0)
    with pytest.raises(ValueError):
        build_model("swin-t", dropout=0.1)
    assert build_model("swin_tiny", 10, drop_path=0.1).stages[3][1].p_path \
        == pytest.approx(0.1)
