"""Depthwise conv on the CPU branch, Conv2dNHWC(groups=...), and the ConvNeXt
wiring (no GPU)."""

import pytest
import torch
import torch.nn.functional as F

import _errbound as eb
from pytorch_ddp_template_amd.ddp import build_parser, main
from pytorch_ddp_template_amd.models import build_model
from pytorch_ddp_template_amd.ops import Conv2dNHWC, conv2d_nhwc


@pytest.mark.parametrize("n,h,w,c,r,pad", [(2, 9, 19, 40, 7, 3),
                                           (2, 9, 9, 16, 3, 0)])
def test_dwconv_cpu_branch_matches_float64(n, h, w, c, r, pad):
    x = eb.randn(n, h, w, c, seed=1).requires_grad_(True)
    wt = eb.randn(c, r, r, 1, seed=2, scale=0.3).requires_grad_(True)
    b = eb.randn(c, seed=3).requires_grad_(True)
    y = conv2d_nhwc(x, wt, b, pad=pad, groups=c)
    dy = eb.randn(*y.shape, seed=4)
    y.backward(dy)
    xd, wd, bd = (t.detach().double().requires_grad_(True) for t in (x, wt, b))
    yd = F.conv2d(xd.permute(0, 3, 1, 2), wd.permute(0, 3, 1, 2), bd, 1, pad,
                  groups=c).permute(0, 2, 3, 1)
    yd.backward(dy.double())
    for got, want in ((y, yd), (x.grad, xd.grad), (wt.grad, wd.grad),
                      (b.grad, bd.grad)):
        torch.testing.assert_close(got.detach().double(), want.detach(),
                                   rtol=1e-4, atol=1e-4)


def test_conv2d_module_groups():
    dense = Conv2dNHWC(16, 32, 3, padding=1, bias=True)
    assert list(dense.state_dict()) == ["weight", "bias"]
    assert dense.weight.shape == (32, 3, 3, 16)
    assert "groups" not in dense.extra_repr()
    dwc = Conv2dNHWC(16, 16, 7, padding=3, groups=16)
    assert dwc.weight.shape == (16, 7, 7, 1)
    assert "groups=16" in dwc.extra_repr()
    assert dwc(torch.zeros(1, 8, 8, 16)).shape == (1, 8, 8, 16)


def test_convnext_tiny_parameter_count():
    dims, depths = (96, 192, 384, 768), (3, 3, 9, 3)
    want = 3 * 16 * dims[0] + dims[0] + 2 * dims[0]          # stem + norm
    for a, b in zip(dims, dims[1:]):
        want += 2 * a + 4 * a * b + b                         # norm + 2x2 conv
    for d, k in zip(dims, depths):
        block = (49 * d + d) + 2 * d + (4 * d * d + 4 * d) + (4 * d * d + d)
        want += k * block
    want += 2 * dims[-1] + dims[-1] * 1000 + 1000             # norm + head
    m = build_model("convnext-t")
    assert sum(p.numel() for p in m.parameters()) == want
    # the published 28.59 M includes 6,624 layer-scale parameters
    assert want + sum(d * k for d, k in zip(dims, depths)) == 28_589_128
    assert m.no_weight_decay() == set()


def test_convnext_cli_arguments():
    args = build_parser().parse_args(
        ["--model", "convnext-t", "--drop_path", "0.1"])
    assert args.drop_path == 0.1
    assert build_model("convnext_tiny", 10, drop_path=0.1).stages[3][2].p_path \
        == pytest.approx(0.1)
    with pytest.raises(SystemExit):
        main(["--model", "convnext-t", "--dropout", "0.1"])
    with pytest.raises(ValueError):
        build_model("convnext-t", dropout=0.1)
    with pytest.raises(ValueError):
        build_model("resnet50", drop_path=0.1)
