"""fp32 GPU path (the command-line default dtype) vs float64 references.

In fp32 the ResNet blocks run unfused: every conv goes through
conv2d_fwd_f32, the zero-stuff dgrad composed in ops.cpp (weight_rot ->
zero_stuff -> conv fwd) and conv2d_wgrad_f32; ViT attention is composed from
the batched fp32 GEMMs.  GEMM-shaped ops are held to the per-element
dot-product bound of _errbound.py, everything else to the tolerance
calibrated against this project's own CPU fp32 branch.
"""

import pytest
import torch
import torch.nn.functional as F

import _errbound as eb

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from pytorch_ddp_template_amd.ops.native import native

    EXT = native()
DEV = "cuda:0"
F32 = torch.float32


def _poison_for(*shape):
    n = 1
    for s in shape:
        n *= s
    eb.poison(DEV, 4 * n)


# ------------------------------------------------------------- conv --------

# (n, h, w, cin, kout, r, stride, pad)
CONV_SHAPES = [
    (2, 8, 16, 4, 10, 3, 1, 1),     # smallest Cin, non-square, Kout % 4 != 0
    (2, 8, 10, 8, 12, 3, 2, 1),     # stem-width Cin, stride 2 + output padding
    (1, 8, 8, 32, 64, 1, 1, 0),     # 1x1
    (2, 8, 8, 64, 72, 1, 2, 0),     # downsample; N-tile tail
    (2, 12, 20, 8, 16, 7, 2, 3),    # 7x7 stem
    (3, 4, 4, 128, 130, 3, 1, 1),   # two J tiles; I-tile tail; M=48 chunk tail
    (2, 6, 6, 24, 16, 3, 1, 1),     # non-pow2 Cin: im2col fallback
]
STEM = CONV_SHAPES[1]


def _conv_inputs(shape):
    n, h, w, cin, kout, r, stride, pad = shape
    ho, wo = eb.conv_out_hw(h, w, r, stride, pad)
    x = eb.randn(n, h, w, cin, seed=101)
    wt = eb.randn(kout, r, r, cin, seed=102, scale=(2.0 / (r * r * cin)) ** 0.5)
    bias = eb.randn(kout, seed=103)
    dy = eb.randn(n, ho, wo, kout, seed=104, scale=0.1)
    return x, wt, bias, dy, ho, wo


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=str)
@pytest.mark.parametrize("epilogue", ["plain", "bias_relu"])
def test_conv2d_fwd_f32(shape, epilogue):
    n, h, w, cin, kout, r, stride, pad = shape
    x, wt, bias, _, ho, wo = _conv_inputs(shape)
    fused = epilogue == "bias_relu"
    b = bias if fused else None
    ref, mag, depth = eb.conv_fwd_ref(x, wt, b, stride, pad, relu=fused)
    _poison_for(n, ho, wo, kout)
    out = EXT.conv2d_fwd(x.to(DEV), wt.to(DEV),
                         None if b is None else b.to(DEV), stride, pad, fused)
    assert out.dtype == F32
    eb.assert_gemm_close(out, ref, mag, depth, f"conv_fwd_f32[{epilogue}]{shape}")


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=str)
def test_conv2d_dgrad_f32(shape):
    n, h, w, cin, kout, r, stride, pad = shape
    _, wt, _, dy, _, _ = _conv_inputs(shape)
    ref, mag, depth = eb.conv_dgrad_ref(dy, wt, stride, pad, h, w)
    _poison_for(n, h, w, cin)
    dx = EXT.conv2d_dgrad(dy.to(DEV), wt.to(DEV), stride, pad, h, w)
    assert dx.dtype == F32
    eb.assert_gemm_close(dx, ref, mag, depth, f"conv_dgrad_f32{shape}")


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=str)
def test_conv2d_wgrad_f32(shape):
    n, h, w, cin, kout, r, stride, pad = shape
    x, _, _, dy, _, _ = _conv_inputs(shape)
    ref, mag, depth = eb.conv_wgrad_ref(dy, x, stride, pad, r, r)
    _poison_for(kout, r, r, cin)
    dw = EXT.conv2d_wgrad(dy.to(DEV), x.to(DEV), stride, pad, r, r)
    assert dw.dtype == F32
    eb.assert_gemm_close(dw, ref, mag, depth, f"conv_wgrad_f32{shape}")


def test_conv2d_nhwc_f32_stem_channel_pad():
    """The 3-channel stem through the autograd op: C is zero-padded 3 -> 8
    for the fast path and dx / dw are sliced back; db is the col_sum."""
    from pytorch_ddp_template_amd.ops.functional import conv2d_nhwc

    n, h, w, _, kout, r, stride, pad = STEM
    cin = 3
    ho, wo = eb.conv_out_hw(h, w, r, stride, pad)
    x = eb.randn(n, h, w, cin, seed=111)
    wt = eb.randn(kout, r, r, cin, seed=112, scale=0.3)
    bias = eb.randn(kout, seed=113)
    dy = eb.randn(n, ho, wo, kout, seed=114, scale=0.1)
    xg = x.to(DEV).requires_grad_(True)
    wg = wt.to(DEV).requires_grad_(True)
    bg = bias.to(DEV).requires_grad_(True)
    _poison_for(n, ho, wo, kout)
    y = conv2d_nhwc(xg, wg, bg, stride, pad)
    y.backward(dy.to(DEV))
    assert xg.grad.shape == x.shape and wg.grad.shape == wt.shape
    eb.assert_gemm_close(y, *eb.conv_fwd_ref(x, wt, bias, stride, pad), "stem y")
    eb.assert_gemm_close(xg.grad, *eb.conv_dgrad_ref(dy, wt, stride, pad, h, w),
                         "stem dx")
    eb.assert_gemm_close(wg.grad, *eb.conv_wgrad_ref(dy, x, stride, pad, r, r),
                         "stem dw")
    d = dy.double().reshape(-1, kout)
    eb.assert_gemm_close(bg.grad, d.sum(0), d.abs().sum(0), d.shape[0], "stem db")


# -------------------------------------------------- batched fp32 GEMMs -----

B_, S_, D_ = 6, 37, 16   # S=37: K pad in bmm_nn, per-batch loop in bmm_tn_f32


def test_bmm_f32_batched():
    q = eb.randn(B_, S_, D_, seed=121)
    k = eb.randn(B_, S_, D_, seed=122)
    p = eb.randn(B_, S_, S_, seed=123)
    _poison_for(B_, S_, S_)
    eb.assert_gemm_close(EXT.bmm_nt(q.to(DEV), k.to(DEV)),
                         *eb.linear_ref(q, k), "bmm_nt_f32")
    _poison_for(B_, S_, D_)
    eb.assert_gemm_close(EXT.bmm_nn(p.to(DEV), k.to(DEV)),
                         *eb.nn_ref(p, k), "bmm_nn_f32 (K=37 padded)")
    _poison_for(B_, S_, D_)
    eb.assert_gemm_close(EXT.bmm_tn(p.to(DEV), q.to(DEV)),
                         *eb.tn_ref(p, q), "bmm_tn_f32 [37x16]")
    _poison_for(B_, D_, S_)
    eb.assert_gemm_close(EXT.bmm_tn(q.to(DEV), p.to(DEV)),
                         *eb.tn_ref(q, p), "bmm_tn_f32 [16x37]")


def test_transpose2d_f32():
    x = eb.randn(5, 70, 33, seed=124)
    _poison_for(5, 70, 33)
    out = EXT.transpose2d(x.to(DEV))
    assert torch.equal(out.cpu(), x.transpose(1, 2).contiguous())


# ------------------------------- non-GEMM fp32 ops via autograd wrappers ---


def _run(fn, inputs, grads, device, dtype, seed=900):
    """Run fn(**inputs) on `device`, backprop a fixed dy through the first
    output; returns {output names, 'd<input>' grads} on the CPU."""
    t = {}
    for k, v in inputs.items():
        if torch.is_tensor(v):
            v = v.to(dtype) if v.is_floating_point() else v
            v = v.clone().to(device)
            if k in grads:
                v.requires_grad_(True)
        t[k] = v
    if device != "cpu":
        eb.poison(device, 1 << 20)
    outs = fn(**t)
    res = {k: v.detach().cpu() for k, v in outs.items()}
    if grads:
        y = next(iter(outs.values()))
        dy = eb.randn(*y.shape, seed=seed).to(dtype)
        y.backward(dy.to(device))
        for k in grads:
            res["d" + k] = t[k].grad.detach().cpu()
    return res


def _check(op, proj_fn, ref_fn, inputs, grads):
    ref = _run(ref_fn, inputs, grads, "cpu", torch.float64)
    cpu = _run(proj_fn, inputs, grads, "cpu", F32)
    gpu = _run(proj_fn, inputs, grads, DEV, F32)
    eb.assert_calibrated(op, gpu, cpu, ref)


def _Fn():
    import pytorch_ddp_template_amd.ops.functional as Fn

    return Fn


@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("act", [None, "relu"])
def test_bn_train_f32(C, act):
    M, mom, eps = 300, 0.1, 1e-5   # 300: no multiple of the block

    def proj(x, g, b, rm, rv):
        y = _Fn().batch_norm2d_nhwc(x, g, b, rm, rv, True, mom, eps, act)
        return {"y": y, "running_mean": rm, "running_var": rv}

    def ref(x, g, b, rm, rv):
        xs = x.reshape(-1, C)
        mean, var = xs.mean(0), xs.var(0, unbiased=False)
        y = (x - mean) * (var + eps).rsqrt() * g + b
        if act == "relu":
            y = torch.relu(y)
        return {"y": y, "running_mean": (1 - mom) * rm + mom * mean.detach(),
                "running_var": (1 - mom) * rv
                + mom * var.detach() * (M / (M - 1))}

    inputs = dict(x=eb.randn(3, 10, 10, C, seed=131) * 2 + 0.5,
                  g=eb.randn(C, seed=132), b=eb.randn(C, seed=133),
                  rm=eb.randn(C, seed=134), rv=eb.randn(C, seed=135).abs() + 0.5)
    _check(f"bn_train[C={C},act={act}]", proj, ref, inputs, ("x", "g", "b"))


@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("act", [None, "relu"])
def test_bn_eval_f32(C, act):
    eps = 1e-5

    def proj(x, g, b, rm, rv):
        return {"y": _Fn().batch_norm2d_nhwc(x, g, b, rm, rv, False, 0.1, eps,
                                             act)}

    def ref(x, g, b, rm, rv):
        y = (x - rm) * (rv + eps).rsqrt() * g + b
        return {"y": torch.relu(y) if act == "relu" else y}

    inputs = dict(x=eb.randn(3, 10, 10, C, seed=136) * 2 + 0.5,
                  g=eb.randn(C, seed=137), b=eb.randn(C, seed=138),
                  rm=eb.randn(C, seed=139), rv=eb.randn(C, seed=140).abs() + 0.5)
    _check(f"bn_eval[C={C},act={act}]", proj, ref, inputs, ())


@pytest.mark.parametrize("D", [40, 768])
def test_layernorm_f32(D):
    def proj(x, g, b):
        return {"y": _Fn().layer_norm(x, g, b, 1e-6)}

    def ref(x, g, b):
        return {"y": F.layer_norm(x, (D,), g, b, 1e-6)}

    inputs = dict(x=eb.randn(33, D, seed=141) * 2 + 0.5,
                  g=eb.randn(D, seed=142), b=eb.randn(D, seed=143))
    _check(f"layernorm[D={D}]", proj, ref, inputs, ("x", "g", "b"))


def test_softmax_f32():
    def proj(x):
        return {"y": _Fn().softmax(x, 0.125)}

    def ref(x):
        return {"y": torch.softmax(x * 0.125, dim=-1)}

    _check("softmax[D=197]", proj, ref,
           dict(x=eb.randn(33, 197, seed=144) * 8), ("x",))


@pytest.mark.parametrize("D", [10, 1000])
def test_cross_entropy_f32(D):
    def proj(logits, target):
        return {"loss": _Fn().cross_entropy(logits, target)}

    def ref(logits, target):
        return {"loss": F.cross_entropy(logits, target)}

    g = torch.Generator().manual_seed(145)
    inputs = dict(logits=eb.randn(33, D, seed=146) * 3,
                  target=torch.randint(0, D, (33,), generator=g))
    _check(f"cross_entropy[D={D}]", proj, ref, inputs, ("logits",))


def test_mse_f32():
    def proj(pred, target):
        return {"loss": _Fn().mse_loss(pred, target)}

    def ref(pred, target):
        return {"loss": F.mse_loss(pred, target)}

    inputs = dict(pred=eb.randn(33, 7, seed=147), target=eb.randn(33, 7, seed=148))
    _check("mse", proj, ref, inputs, ("pred",))


def test_pools_f32_nonsquare():
    x = eb.randn(3, 8, 12, 16, seed=149)

    def avg_ref(x):
        return {"y": x.mean(dim=(1, 2))}

    def max_ref(x):
        y = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1)
        return {"y": y.permute(0, 2, 3, 1)}

    _check("avgpool_global", lambda x: {"y": _Fn().global_avg_pool_nhwc(x)},
           avg_ref, dict(x=x), ("x",))
    # the gradient covers the saved index tensor
    _check("maxpool_3_2_1", lambda x: {"y": _Fn().max_pool2d_nhwc(x, 3, 2, 1)},
           max_ref, dict(x=x), ("x",))


def test_elementwise_f32():
    a = eb.randn(1001, seed=150)
    b = eb.randn(1001, seed=151)
    _check("relu", lambda x: {"y": _Fn().relu(x)},
           lambda x: {"y": torch.relu(x)}, dict(x=a), ("x",))
    _check("add_relu", lambda a, b: {"y": _Fn().add_relu(a, b)},
           lambda a, b: {"y": torch.relu(a + b)}, dict(a=a, b=b), ("a", "b"))
    _check("gelu", lambda x: {"y": _Fn().gelu(x)},
           lambda x: {"y": F.gelu(x)}, dict(x=a * 2), ("x",))


def test_col_sum_f32():
    dy = eb.randn(1000, 65, seed=152)
    eb.poison(DEV, 4 * 65)
    gpu = {"y": EXT.col_sum(dy.to(DEV)).cpu()}
    # functional.py's CPU branch of the bias grad is a plain fp32 sum
    eb.assert_calibrated("col_sum", gpu, {"y": dy.sum(0)},
                         {"y": dy.double().sum(0)})


def test_attention_composed_f32():
    """softmax(q k^T * scale) v composed from bmm_nt / softmax / bmm_nn, and
    its backward (bmm_nn, bmm_tn, softmax_bwd)."""
    def proj(q, k, v):
        return {"out": _Fn().attention(q, k, v, 0.25)}

    def ref(q, k, v):
        p = torch.softmax(q @ k.transpose(1, 2) * 0.25, dim=-1)
        return {"out": p @ v}

    inputs = dict(q=eb.randn(B_, S_, D_, seed=153), k=eb.randn(B_, S_, D_, seed=154),
                  v=eb.randn(B_, S_, D_, seed=155))
    _check("attention", proj, ref, inputs, ("q", "k", "v"))
