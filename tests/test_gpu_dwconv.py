"""Depthwise conv kernels (ops/csrc/dwconv.hip) against float64 within the
bound of _errbound.py, and the ConvNeXt model built on them.  (3,16,33,96,7,3)
is already 2x2 forward tiles and 12 wgrad partials per slab: not enlarged."""

import copy

import pytest
import torch
import torch.nn.functional as F

import _errbound as eb
from pytorch_ddp_template_amd.ops import CrossEntropyLoss, conv2d_nhwc
from pytorch_ddp_template_amd.ops.native import native as _ext

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (n, h, w, c, r, pad, bias, also fp32)
SHAPES = [
    (1, 1, 1, 8, 7, 3, False, False),
    (2, 7, 7, 32, 7, 3, False, True),
    (2, 9, 19, 40, 7, 3, True, False),
    (3, 16, 33, 96, 7, 3, False, True),
    (2, 12, 10, 16, 3, 1, False, False),
    (2, 10, 12, 24, 5, 2, False, False),
    (2, 9, 9, 16, 3, 0, False, False),
]
CASES = [
    pytest.param(s, dt, id=f"{'x'.join(map(str, s[:6]))}-{str(dt)[6:]}")
    for s in SHAPES
    for dt in (torch.bfloat16, torch.float16, torch.float32)
    if dt != torch.float32 or s[7]
]


def _inputs(shape, dtype):
    n, h, w, c, r, pad, bias, _ = shape
    ho, wo = eb.conv_out_hw(h, w, r, 1, pad)
    x = eb.randn(n, h, w, c, seed=1, dtype=dtype)
    wt = eb.randn(c, r, r, 1, seed=2, scale=0.3, dtype=dtype)
    b = eb.randn(c, seed=3, dtype=dtype) if bias else None
    dy = eb.randn(n, ho, wo, c, seed=4, dtype=dtype)
    return x, wt, b, dy


_nchw, _nhwc = eb._nchw, eb._nhwc


def _ref(op, *ts):
    """(ref, mag): op in float64 on the inputs and on their magnitudes."""
    d = [None if t is None else t.double() for t in ts]
    return op(*d), op(*[None if t is None else t.abs() for t in d])


def _fwd_ref(x, w, b, pad):
    return _ref(lambda a, k, bb: _nhwc(F.conv2d(
        _nchw(a), _nchw(k), bb, 1, pad, groups=a.shape[-1])), x, w, b)


def _dgrad_ref(dy, w, pad, h, wd):
    return _ref(lambda g, k: _nhwc(torch.nn.grad.conv2d_input(
        (g.shape[0], g.shape[-1], h, wd), _nchw(k), _nchw(g), 1, pad,
        groups=g.shape[-1])), dy, w)


def _wgrad_ref(dy, x, pad, r):
    return _ref(lambda g, a: _nhwc(torch.nn.grad.conv2d_weight(
        _nchw(a), (a.shape[-1], 1, r, r), _nchw(g), 1, pad,
        groups=a.shape[-1])), dy, x)


@pytest.mark.parametrize("shape,dtype", CASES)
def test_dwconv_fwd(shape, dtype):
    x, w, b, _ = _inputs(shape, dtype)
    r, pad = shape[4], shape[5]
    ref, mag = _fwd_ref(x, w, b, pad)
    eb.poison(DEV, ref.numel() * 4)
    out = _ext().dwconv2d_fwd(x.to(DEV), w.to(DEV),
                              None if b is None else b.to(DEV), pad)
    eb.assert_gemm_close(out, ref, mag, r * r, "dwconv2d_fwd")


@pytest.mark.parametrize("shape,dtype", CASES)
def test_dwconv_dgrad(shape, dtype):
    _, w, _, dy = _inputs(shape, dtype)
    h, wd, r, pad = shape[1], shape[2], shape[4], shape[5]
    ref, mag = _dgrad_ref(dy, w, pad, h, wd)
    eb.poison(DEV, ref.numel() * 4)
    out = _ext().dwconv2d_dgrad(dy.to(DEV), w.to(DEV), pad, h, wd)
    eb.assert_gemm_close(out, ref, mag, r * r, "dwconv2d_dgrad")


@pytest.mark.parametrize("shape,dtype", CASES)
def test_dwconv_wgrad(shape, dtype):
    x, _, _, dy = _inputs(shape, dtype)
    r, pad = shape[4], shape[5]
    ref, mag = _wgrad_ref(dy, x, pad, r)
    eb.poison(DEV, 1 << 20)
    out = _ext().dwconv2d_wgrad(dy.to(DEV), x.to(DEV), pad, r)
    assert out.dtype == torch.float32
    eb.assert_gemm_close(out, ref, mag, dy.shape[0] * dy.shape[1] * dy.shape[2],
                         "dwconv2d_wgrad", out_dtype=torch.float32)
    if shape[1] == 1 and shape[2] == 1:  # only the centre tap sees the pixel
        dead = torch.ones(r, r, dtype=torch.bool)
        dead[pad, pad] = False
        assert (out.cpu()[:, dead] == 0).all()


def test_dwconv_autograd():
    shape, dtype = SHAPES[2], torch.bfloat16
    x, w, b, dy = _inputs(shape, dtype)
    n, h, wd, c, r, pad = shape[:6]
    xg, wg, bg = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    y = conv2d_nhwc(xg, wg, bg, pad=pad, groups=c)
    y.backward(dy.to(DEV))
    eb.assert_gemm_close(y, *_fwd_ref(x, w, b, pad), r * r, "autograd y")
    eb.assert_gemm_close(xg.grad, *_dgrad_ref(dy, w, pad, h, wd), r * r,
                         "autograd dx")
    # dw and db are fp32 sums rounded once to the parameter's dtype
    m = dy.shape[0] * dy.shape[1] * dy.shape[2]
    eb.assert_gemm_close(wg.grad, *_wgrad_ref(dy, x, pad, r), m, "autograd dw")
    dyd = dy.double()
    eb.assert_gemm_close(bg.grad, dyd.sum((0, 1, 2)), dyd.abs().sum((0, 1, 2)),
                         m, "autograd db")


@pytest.mark.parametrize("c,kw", [(16, dict(groups=2)),
                                  (16, dict(groups=16, stride=2)),
                                  (12, dict(groups=12))])
def test_dwconv_errors(c, kw):
    x = torch.zeros(1, 8, 8, c, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(c, 3, 3, c // kw["groups"], device=DEV, dtype=torch.bfloat16)
    with pytest.raises((ValueError, RuntimeError)):
        conv2d_nhwc(x, w, None, pad=1, **kw)


def test_dwconv_wgrad_repeatable():
    x, _, _, dy = _inputs(SHAPES[3], torch.bfloat16)
    x, dy = x.to(DEV), dy.to(DEV)
    a = _ext().dwconv2d_wgrad(dy, x, 3, 7)
    b = _ext().dwconv2d_wgrad(dy, x, 3, 7)
    assert torch.equal(a, b)


def _tiny_convnext():
    from pytorch_ddp_template_amd.models.convnext import ConvNeXt

    torch.manual_seed(5)
    return ConvNeXt((1, 1, 1, 1), (16, 32, 48, 64), num_classes=10)


def test_convnext_bf16_close_to_cpu_f32():
    m = _tiny_convnext()
    mg = copy.deepcopy(m).to(torch.bfloat16).to(DEV)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(4, 32, 32, 3, generator=g)
    y = torch.randint(0, 10, (4,), generator=g)
    ref = m(x)
    CrossEntropyLoss()(ref, y).backward()
    out = mg(x.to(torch.bfloat16).to(DEV))
    CrossEntropyLoss()(out, y.to(DEV)).backward()
    pairs = {
        "logits": (out, ref),
        "dw weight": (mg.stages[0][0].dwconv.weight.grad,
                      m.stages[0][0].dwconv.weight.grad),
        "stem weight": (mg.downsample[0][0].weight.grad,
                        m.downsample[0][0].weight.grad),
    }
    for name, (got, want) in pairs.items():
        err = (got.detach().float().cpu() - want.detach()).abs().max()
        scale = want.detach().abs().max().clamp(min=1.0 if name == "logits" else 0)
        print(f"CONVNEXT {name} err/scale={float(err / scale):.4f}")
        # the bound of test_gpu_models.py
        # test_resnet18_bf16_forward_close_to_cpu_f32 for bf16 model outputs
        assert err / scale < 0.12, f"{name}: relative error {err / scale}"


def test_convnext_step_under_graph_capture():
    from pytorch_ddp_template_amd.optim import SGD

    m = _tiny_convnext().to(torch.bfloat16).to(DEV)
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9, master_weights=True)
    crit = CrossEntropyLoss()
    g = torch.Generator().manual_seed(7)
    x = torch.randn(4, 32, 32, 3, generator=g).to(torch.bfloat16).to(DEV)
    y = torch.randint(0, 10, (4,), generator=g).to(DEV)

    lr_dev = torch.full((), 0.05, dtype=torch.float32, device=DEV)

    def step():
        loss = crit(m(x), y)
        loss.backward()
        opt.step(lr_tensor=lr_dev)
        m.zero_grad(set_to_none=False)
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):  # the capture recipe of bench.py
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        loss = step()
    losses = []
    for _ in range(3):
        graph.replay()
        losses.append(float(loss))
    assert all(v == v and abs(v) < 1e4 for v in losses), losses
    assert len(set(losses)) == 3, losses
