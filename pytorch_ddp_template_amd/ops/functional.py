"""Autograd-wrapped ops backed by hand-written CDNA4 HIP kernels.

Every op in this file has two execution paths:

* **GPU (ROCm)** — the in-tree HIP extension (``ops/csrc``): MFMA + LDS-tiled
  kernels for the GEMM-shaped work, fused elementwise/normalization kernels
  for the bandwidth-bound work.  If the extension is missing on a GPU box the
  op raises (no silent eager fallback).
* **CPU** — plain PyTorch reference implementations.  These are the numerics
  references the HIP kernels are tested against, and they make the whole
  training loop runnable hardware-free (the reference template's
  ``--no_cuda`` property, reference ddp.py:90-95).

Conventions:

* Conv/pool/norm tensors are **NHWC** ``(N, H, W, C)`` plain-contiguous — the
  MI355X-friendly layout (C-contiguous rows feed MFMA K-contiguous fragments
  and coalesced 16 B/lane loads).
* Linear weights are ``(out_features, in_features)`` (torch convention) which
  is already the K-contiguous "NT" GEMM operand.
* Conv weights are ``(K_out, R, S, C_in)`` ("KRSC") — K-contiguous for the
  implicit-GEMM forward.
* Kernels accumulate in fp32 regardless of I/O dtype (bf16 or fp32).

Reference parity: these ops cover the compute inventory of SURVEY.md §2b
(reference model.py:11-16 Linear/ReLU, ddp.py:164 MSELoss, ddp.py:238-240
clip+SGD) plus the conv/BN/CE/pool/LN/attention set required by the
ResNet/ViT benchmark configs.
"""

from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import fused_block, rng
from .native import native, use_native

# ---------------------------------------------------------------------------
# Linear (+ optional fused ReLU epilogue)
# ---------------------------------------------------------------------------


# Transposed-operand wgrad route: measured SLOWER than the TN kernels on
# the ViT shapes (NT-T 271-338 TF vs TN 425-496; ViT bench 3,116 vs 3,987
# samples/s) — the two explicit transposes plus the split-K z-chunking
# (each block runs only ~14 K-tiles, back in the pipeline-fill-dominated
# regime) cost more than the transpose-free staging saves.  Kept behind
# PDT_WGRAD_NT=1 as a documented negative result.
_WGRAD_NT = os.environ.get("PDT_WGRAD_NT", "0") == "1"


def _wgrad_via_nt(dys, xs) -> bool:
    return (
        _WGRAD_NT
        and dys.dtype == torch.bfloat16
        and dys.shape[0] >= 4096
        and dys.shape[0] % 64 == 0
        and dys.shape[1] % 256 == 0
        and xs.shape[1] % 256 == 0
    )


def _plain_gemm_to_blas(m: int, k: int, n: int) -> bool:
    """Big plain GEMMs go to rocBLAS/hipBLASLt (the MI355X library path,
    sanctioned for PLAIN library GEMMs only); every fused shape (bias/relu
    epilogues, conv modes, bias-grad-in-GEMM) stays on the hand-written
    kernels.  Round-2 status (tools/plain256_ab.py, 1xMI355X): the new
    256x256-tile glds kernel (ops/csrc/gemm_plain.hip) reaches 1040-1130 TF
    sustained and 870-960 TF on the ViT-B/16 linear shapes — up from
    510-687 TF in round 1 — vs rocBLAS 950-1150 on the same box, so the
    library keeps a measured ~10% edge on exactly these shapes and keeps
    the route.  Pipelined variants (counted-vmcnt k-half phases, 3-buffer
    ring, 32x32 MFMA) all measured slower than the simple 2-buffer glds
    structure; the remaining gap is the barrier's glds drain, which per the
    CDNA4 guide only the exact asm-level 8-phase interleave removes.
    """
    return m >= 4096 and k >= 512 and n >= 512


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, act):
        # x: (..., K) ; w: (N, K) ; b: (N,) or None
        xs = x.reshape(-1, x.shape[-1])
        if use_native(x, w) and _plain_gemm_to_blas(
            xs.shape[0], xs.shape[1], w.shape[0]
        ):
            y = torch.nn.functional.linear(xs.contiguous(), w, b)
            if act == "relu":
                y = torch.relu(y)
        elif use_native(x, w):
            y = native().gemm_nt(xs.contiguous(), w, b, act == "relu", False)
        else:
            y = xs @ w.t()
            if b is not None:
                y = y + b
            if act == "relu":
                y = torch.relu(y)
        y = y.reshape(*x.shape[:-1], w.shape[0])
        ctx.save_for_backward(x, w, y if act == "relu" else None)
        ctx.act = act
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y_relu = ctx.saved_tensors
        dys = dy.reshape(-1, dy.shape[-1]).contiguous()
        xs = x.reshape(-1, x.shape[-1]).contiguous()
        if use_native(dy, w):
            ext = native()
            if ctx.act == "relu":
                dys = ext.relu_bwd(dys, y_relu.reshape_as(dys))
            if _plain_gemm_to_blas(dys.shape[0], dys.shape[1], w.shape[1]):
                dx = dys @ w  # rocBLAS NN, no w-transpose materialization
            else:
                wt = ext.transpose2d(w)  # (K, N)
                dx = ext.gemm_nt(dys, wt, None, False, False)
            if _wgrad_via_nt(dys, xs):
                # transposed-operand route (gemm_plain.hip split-K NT):
                # transposing dy and x once (two HBM passes over tensors the
                # wgrad reads anyway) turns the TN wgrad into a plain NT
                # GEMM with the huge M as reduction — the glds kernel's
                # best regime (TN kernels cap at ~450-530 TF on these
                # shapes; ViT wgrad was 29% of the step)
                dyT = ext.transpose2d(dys)
                xT = ext.transpose2d(xs)
                dw = ext.gemm_nt_splitk_f32(dyT, xT).to(w.dtype)
                db = ext.col_sum(dys).to(w.dtype) if ctx.has_bias else None
            elif ctx.has_bias and dys.dtype in (torch.bfloat16, torch.float16):
                # bias grad rides inside the TN GEMM (dy is staged anyway)
                dwf, dbf = ext.gemm_tn_bias(dys, xs)
                dw = dwf.to(w.dtype)
                db = dbf.to(w.dtype)
            else:
                dw = ext.gemm_tn(dys, xs).to(w.dtype)
                db = ext.col_sum(dys).to(w.dtype) if ctx.has_bias else None
        else:
            if ctx.act == "relu":
                dys = dys * (y_relu.reshape_as(dys) > 0).to(dys.dtype)
            dx = dys @ w
            dw = (dys.t().to(torch.float32) @ xs.to(torch.float32)).to(w.dtype)
            db = dys.sum(0).to(w.dtype) if ctx.has_bias else None
        return dx.reshape_as(x), dw, db, None


def linear(x, w, b=None, act=None):
    return _LinearFn.apply(x, w, b, act)


# ---------------------------------------------------------------------------
# ReLU / residual add-ReLU
# ---------------------------------------------------------------------------


class _ReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        if use_native(x):
            y = native().relu_fwd(x.contiguous())
        else:
            y = torch.relu(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        if use_native(dy):
            return native().relu_bwd(dy.contiguous(), y)
        return dy * (y > 0).to(dy.dtype)


def relu(x):
    return _ReluFn.apply(x)


class _AddReluFn(torch.autograd.Function):
    """Fused residual add + ReLU (ResNet block tail)."""

    @staticmethod
    def forward(ctx, a, b):
        if use_native(a, b):
            y = native().add_relu_fwd(a.contiguous(), b.contiguous())
        else:
            y = torch.relu(a + b)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        if use_native(dy):
            da = native().relu_bwd(dy.contiguous(), y)
        else:
            da = dy * (y > 0).to(dy.dtype)
        return da, da


def add_relu(a, b):
    return _AddReluFn.apply(a, b)


# ---------------------------------------------------------------------------
# Conv2d NHWC (implicit GEMM)
# ---------------------------------------------------------------------------


def _conv_ref_nhwc(x, w, b, stride, pad):
    # CPU reference through torch's NCHW conv.
    xc = x.permute(0, 3, 1, 2).float()
    wc = w.permute(0, 3, 1, 2).float()  # (K, C, R, S)
    y = F.conv2d(xc, wc, b.float() if b is not None else None, stride, pad)
    return y.permute(0, 2, 3, 1).contiguous().to(x.dtype)


class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, pad, act):
        cpad = 0
        if use_native(x, w):
            C = x.shape[-1]
            if C < 8:
                # narrow input (the 3-channel stem): zero-pad channels to 8
                # so the fast implicit-GEMM path applies instead of
                # materializing a huge im2col (740 MB for ResNet-50's stem)
                cpad = 8 - C
                x = torch.nn.functional.pad(x, (0, cpad))
                w = torch.nn.functional.pad(w, (0, cpad))
            y = native().conv2d_fwd(
                x.contiguous(), w.contiguous(), b, stride, pad, act == "relu"
            )
        else:
            y = _conv_ref_nhwc(x, w, b, stride, pad)
            if act == "relu":
                y = torch.relu(y)
        ctx.save_for_backward(x, w, y if act == "relu" else None)
        ctx.meta = (stride, pad, act, b is not None, cpad)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y_relu = ctx.saved_tensors
        stride, pad, act, has_bias, cpad = ctx.meta
        dy = dy.contiguous()
        if use_native(dy, w):
            ext = native()
            if act == "relu":
                dy = ext.relu_bwd(dy, y_relu)
            dx = (
                ext.conv2d_dgrad(dy, w, stride, pad, x.shape[1], x.shape[2])
                if ctx.needs_input_grad[0]
                else None
            )
            dw = ext.conv2d_wgrad(dy, x, stride, pad, w.shape[1], w.shape[2]).to(
                w.dtype
            )
            db = (
                ext.col_sum(dy.reshape(-1, dy.shape[-1])).to(w.dtype)
                if has_bias
                else None
            )
        else:
            if act == "relu":
                dy = dy * (y_relu > 0).to(dy.dtype)
            dyc = dy.permute(0, 3, 1, 2).float()
            xc = x.permute(0, 3, 1, 2).float()
            wc = w.permute(0, 3, 1, 2).float()
            dxc = torch.nn.grad.conv2d_input(xc.shape, wc, dyc, stride, pad)
            dwc = torch.nn.grad.conv2d_weight(xc, wc.shape, dyc, stride, pad)
            dx = dxc.permute(0, 2, 3, 1).contiguous().to(x.dtype)
            dw = dwc.permute(0, 2, 3, 1).contiguous().to(w.dtype)
            db = dy.sum(dim=(0, 1, 2)).to(w.dtype) if has_bias else None
        if cpad:
            # saved x/w were channel-padded for the stem fast path: un-slice
            # dw/dx back to the caller's channel count in BOTH branches (the
            # fallback branch computed grads against the padded tensors too).
            dw = dw[..., : w.shape[-1] - cpad].contiguous()
            if dx is not None:
                dx = dx[..., : w.shape[-1] - cpad].contiguous()
        return dx, dw, db, None, None, None


class _DwConv2dFn(torch.autograd.Function):
    """Depthwise conv, stride 1: x (N, H, W, C), w (C, R, R, 1).  GPU: the
    dw:: kernels of ops/csrc/dwconv.hip (the data gradient is the forward
    kernel with reversed taps, the weight gradient a two-stage fixed-order
    reduction).  CPU: torch's grouped conv in fp32."""

    @staticmethod
    def forward(ctx, x, w, b, pad):
        if use_native(x, w):
            y = native().dwconv2d_fwd(x.contiguous(), w.contiguous(), b, pad)
        else:
            C = x.shape[-1]
            y = F.conv2d(
                x.permute(0, 3, 1, 2).float(), w.permute(0, 3, 1, 2).float(),
                b.float() if b is not None else None, 1, pad, groups=C)
            y = y.permute(0, 2, 3, 1).contiguous().to(x.dtype)
        ctx.save_for_backward(x, w)
        ctx.meta = (pad, b is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        pad, has_bias = ctx.meta
        dy = dy.contiguous()
        C, R = x.shape[-1], w.shape[1]
        if use_native(dy, w):
            ext = native()
            dx = (
                ext.dwconv2d_dgrad(dy, w.contiguous(), pad, x.shape[1],
                                   x.shape[2])
                if ctx.needs_input_grad[0]
                else None
            )
            dw = (
                ext.dwconv2d_wgrad(dy, x.contiguous(), pad, R).to(w.dtype)
                if ctx.needs_input_grad[1]
                else None
            )
            db = (
                ext.col_sum(dy.reshape(-1, C)).to(w.dtype)
                if has_bias and ctx.needs_input_grad[2]
                else None
            )
        else:
            dyc = dy.permute(0, 3, 1, 2).float()
            xc = x.permute(0, 3, 1, 2).float()
            wc = w.permute(0, 3, 1, 2).float()
            dxc = torch.nn.grad.conv2d_input(xc.shape, wc, dyc, 1, pad, groups=C)
            dwc = torch.nn.grad.conv2d_weight(xc, wc.shape, dyc, 1, pad,
                                              groups=C)
            dx = dxc.permute(0, 2, 3, 1).contiguous().to(x.dtype)
            dw = dwc.permute(0, 2, 3, 1).contiguous().to(w.dtype)
            db = dy.sum(dim=(0, 1, 2)).to(w.dtype) if has_bias else None
        return dx, dw, db, None


def conv2d_nhwc(x, w, b=None, stride=1, pad=0, act=None, groups=1):
    """groups == 1: the dense implicit-GEMM routes.  groups == C == K with
    w (C, R, R, 1): depthwise, R in {3, 5, 7}, stride 1, no fused activation
    (and C % 8 == 0 on the GPU).  Any other grouping is an error."""
    if groups == 1:
        return _Conv2dFn.apply(x, w, b, stride, pad, act)
    C = x.shape[-1]
    if not (groups == C == w.shape[0] and w.shape[-1] == 1):
        raise ValueError(
            f"conv2d_nhwc: groups={groups} with x channels {C} and weight "
            f"{tuple(w.shape)}: only groups == 1 and depthwise "
            "(groups == C == K, one input channel per group) are implemented")
    if stride != 1 or act is not None:
        raise ValueError("conv2d_nhwc: depthwise needs stride 1 and no act")
    if w.shape[1] != w.shape[2] or w.shape[1] not in (3, 5, 7):
        raise ValueError(
            "conv2d_nhwc: depthwise taps must be square 3, 5 or 7, got "
            f"{tuple(w.shape[1:3])}")
    if not 0 <= pad <= w.shape[1] - 1:
        raise ValueError(f"conv2d_nhwc: depthwise pad {pad} not in [0, R-1]")
    return _DwConv2dFn.apply(x, w, b, pad)


# ---------------------------------------------------------------------------
# BatchNorm2d NHWC (optionally fused ReLU)
# ---------------------------------------------------------------------------


class _BatchNorm2dFn(torch.autograd.Function):
    """``offer``: this BN+ReLU feeds a wired fused block and nothing else (the
    CIFAR ResNet stem).  On the native training path its node then makes the
    offer a fused block's node makes (ops/fused_block.py): the consumer may
    mask the gradient it returns by this ReLU and leave the BN-backward sums
    on the node, and the backward runs ``bn_bwd_ws`` on that gradient."""

    @staticmethod
    def forward(
        ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps,
        act, offer=False,
    ):
        C = x.shape[-1]
        xs = x.reshape(-1, C)
        ctx.dy_premasked = None
        if (offer and training and act == "relu" and use_native(x, gamma)
                and x.is_contiguous()
                and fused_block._use_dgrad_epilogue()
                and fused_block._use_dgrad_handoff_bnstats()):
            ctx.dy_premasked = False
        if use_native(x, gamma):
            ext = native()
            if training:
                y, mean, rstd = ext.bn_fwd(
                    xs.contiguous(),
                    gamma,
                    beta,
                    running_mean,
                    running_var,
                    momentum,
                    eps,
                    act == "relu",
                )
            else:
                y = ext.bn_infer(
                    xs.contiguous(),
                    gamma,
                    beta,
                    running_mean,
                    running_var,
                    eps,
                    act == "relu",
                )
                mean = rstd = None
        else:
            xf = xs.float()
            if training:
                mean = xf.mean(0)
                var = xf.var(0, unbiased=False)
                rstd = (var + eps).rsqrt()
                if running_mean is not None:
                    m = xs.shape[0]
                    unbiased = var * (m / max(1, m - 1))
                    running_mean.mul_(1 - momentum).add_(momentum * mean)
                    running_var.mul_(1 - momentum).add_(momentum * unbiased)
            else:
                mean = running_mean.float()
                rstd = (running_var.float() + eps).rsqrt()
            y = (xf - mean) * rstd * gamma.float() + beta.float()
            if act == "relu":
                y = torch.relu(y)
            y = y.to(x.dtype)
        if ctx.dy_premasked is not None:
            fused_block._offer_bn_sums(ctx, x, mean, rstd)
        ctx.save_for_backward(
            x, gamma, mean, rstd, y if act == "relu" else None
        )
        ctx.meta = (training, act)
        return y.reshape_as(x)

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd, y_relu = ctx.saved_tensors
        training, act = ctx.meta
        if not training:
            raise RuntimeError("backward through eval-mode batchnorm is unsupported")
        C = x.shape[-1]
        dys = dy.reshape(-1, C).contiguous()
        xs = x.reshape(-1, C)
        if use_native(dy, gamma):
            ext = native()
            # fused relu mask: bn_bwd applies (y_relu > 0) inline — no
            # separate relu_bwd pass over the tensor
            yr = y_relu.reshape(-1, C) if act == "relu" else None
            ws = fused_block._take_bn_ws(ctx)
            if ws is not None:
                # dy carries the ReLU mask, ws its sums (handed over)
                dx, dgamma, dbeta = ext.bn_bwd_ws(
                    dys, xs.contiguous(), gamma, mean, rstd, ws
                )
            else:
                dx, dgamma, dbeta = ext.bn_bwd(
                    dys, xs.contiguous(), gamma, mean, rstd,
                    None if ctx.dy_premasked else yr
                )
            dgamma = dgamma.to(gamma.dtype)
            dbeta = dbeta.to(gamma.dtype)
        else:
            if act == "relu":
                dys = dys * (y_relu.reshape(-1, C) > 0).to(dys.dtype)
            xf = xs.float()
            dyf = dys.float()
            m = xs.shape[0]
            xhat = (xf - mean) * rstd
            dgamma_f = (dyf * xhat).sum(0)
            dbeta_f = dyf.sum(0)
            dx = (
                (gamma.float() * rstd / m)
                * (m * dyf - dbeta_f - xhat * dgamma_f)
            ).to(x.dtype)
            dgamma = dgamma_f.to(gamma.dtype)
            dbeta = dbeta_f.to(gamma.dtype)
        return (
            dx.reshape_as(x),
            dgamma,
            dbeta,
            None,
            None,
            None,
            None,
            None,
            None,
            None,
        )


def batch_norm2d_nhwc(
    x,
    gamma,
    beta,
    running_mean=None,
    running_var=None,
    training=True,
    momentum=0.1,
    eps=1e-5,
    act=None,
    offer=False,
):
    return _BatchNorm2dFn.apply(
        x, gamma, beta, running_mean, running_var, training, momentum, eps, act,
        offer,
    )


# ---------------------------------------------------------------------------
# Losses
# ---------------------------------------------------------------------------


class _CrossEntropyFn(torch.autograd.Function):
    """Fused log-softmax + NLL (mean reduction), fp32 accumulation."""

    @staticmethod
    def forward(ctx, logits, target):
        if use_native(logits):
            loss, lse = native().ce_fwd(logits.contiguous(), target)
        else:
            lf = logits.float()
            lse = torch.logsumexp(lf, dim=1)
            loss = (lse - lf.gather(1, target[:, None]).squeeze(1)).mean()
        ctx.save_for_backward(logits, target, lse)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, target, lse = ctx.saved_tensors
        if use_native(logits):
            # dloss is passed as a device tensor so backward never forces a
            # host sync (the reference's per-step loss.item() stall,
            # SURVEY.md §3.2, is deliberately avoided).
            dl = native().ce_bwd(
                logits.contiguous(), target, lse, dloss.to(logits.device)
            )
        else:
            scale = float(dloss) / logits.shape[0]
            sm = torch.softmax(logits.float(), dim=1)
            sm[torch.arange(logits.shape[0], device=logits.device), target] -= 1.0
            dl = (sm * scale).to(logits.dtype)
        return dl, None


def _mix_params(mix, device):
    """The 8-slot record of a BatchMix (or the tensor itself) on device."""
    if mix is None or isinstance(mix, torch.Tensor):
        return mix
    return mix.params(device)


class _SoftCrossEntropyFn(torch.autograd.Function):
    """Cross-entropy against the soft target
    q_d = eps/D + (1-eps) (lam [d == t_m] + (1-lam) [d == t_{M-1-m}]),
    mean reduction.  lam is slot 0 of the mix params record (None: 1), read on
    the device by both kernels; q is never built on the GPU.  Forward and
    backward see the same record: only the next step's draw writes it."""

    @staticmethod
    def forward(ctx, logits, target, eps, params):
        if use_native(logits):
            loss, lse = native().ce_soft_fwd(
                logits.contiguous(), target.contiguous(), eps, params)
        else:
            lf = logits.float()
            lse = torch.logsumexp(lf, dim=1)
            q = _soft_target(lf, target, eps, params)
            loss = (lse - (q * lf).sum(1)).mean()
        ctx.save_for_backward(logits, target, lse)
        ctx.eps, ctx.params = eps, params
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, target, lse = ctx.saved_tensors
        if use_native(logits):
            dl = native().ce_soft_bwd(
                logits.contiguous(), target.contiguous(), lse,
                dloss.to(logits.device), ctx.eps, ctx.params)
        else:
            lf = logits.float()
            q = _soft_target(lf, target, ctx.eps, ctx.params)
            scale = float(dloss) / logits.shape[0]
            dl = ((torch.softmax(lf, dim=1) - q) * scale).to(logits.dtype)
        return dl, None, None, None


def _soft_target(lf, target, eps, params):
    """CPU path: the [M, D] float32 soft target."""
    lam = 1.0 if params is None else float(params[0])
    D = lf.shape[1]
    onehot = F.one_hot(target, D).float()
    q = lam * onehot + (1.0 - lam) * onehot.flip(0)
    return eps / D + (1.0 - eps) * q


def cross_entropy(logits, target, label_smoothing=0.0, mix=None):
    """Mean cross-entropy of [M, D] logits against int64 targets [M].

    label_smoothing: weight eps of the uniform distribution in the target.
    mix: a ``BatchMix`` (or its params tensor) whose last draw mixed the batch;
    row m's target is then lam of its own label plus (1 - lam) of the label of
    row M-1-m.  With the defaults this is the hard-label kernel pair."""
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(
            f"label_smoothing must be in [0, 1), got {label_smoothing}")
    if label_smoothing == 0 and mix is None:
        return _CrossEntropyFn.apply(logits, target)
    return _SoftCrossEntropyFn.apply(
        logits, target, float(label_smoothing),
        _mix_params(mix, logits.device))


def batch_mix_(x, mix):
    """Mix the image batch x in place under the record of ``mix`` (a
    ``BatchMix`` or its params tensor): sample i takes the box of, or blends
    with, sample B-1-i.  x: contiguous 4-D, NHWC or (3 channels first) NCHW,
    told apart as the models do."""
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("batch_mix_: x must be a contiguous 4-D image batch")
    params = _mix_params(mix, x.device)
    nchw = x.shape[1] == 3 and x.shape[-1] != 3
    H, W = (x.shape[2], x.shape[3]) if nchw else (x.shape[1], x.shape[2])
    if use_native(x):
        return native().mix_batch_(x, params, H, W, 1 if nchw else x.shape[3])
    ints = params.view(torch.int32)
    if int(ints[6]) == rng.MIX_NONE:
        return x
    a = float(params[1])
    y0, y1, x0, x1 = (int(v) for v in ints[2:6])
    xp = x.flip(0)
    out = x.clone() if a == 1.0 else (
        a * x.float() + (1.0 - a) * xp.float()).to(x.dtype)
    box = (slice(None), slice(None), slice(y0, y1), slice(x0, x1)) if nchw \
        else (slice(None), slice(y0, y1), slice(x0, x1))
    out[box] = xp[box]
    B = x.shape[0]
    if B % 2:
        out[B // 2] = x[B // 2]
    return x.copy_(out)


class _MSEFn(torch.autograd.Function):
    """mean((pred - target)^2) — the reference's criterion (ddp.py:164)."""

    @staticmethod
    def forward(ctx, pred, target):
        ctx.save_for_backward(pred, target)
        if use_native(pred, target):
            return native().mse_fwd(pred.contiguous(), target.contiguous())
        return F.mse_loss(pred.float(), target.float())

    @staticmethod
    def backward(ctx, dloss):
        pred, target = ctx.saved_tensors
        if use_native(pred, target):
            # scale = 2*dloss/numel computed on-device (no host sync).
            dp = native().mse_bwd(
                pred.contiguous(), target.contiguous(), dloss.to(pred.device)
            )
        else:
            scale = 2.0 * float(dloss) / pred.numel()
            dp = (scale * (pred.float() - target.float())).to(pred.dtype)
        return dp, None


def mse_loss(pred, target):
    return _MSEFn.apply(pred, target)


# ---------------------------------------------------------------------------
# Pooling (NHWC)
# ---------------------------------------------------------------------------


class _GlobalAvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        N, H, W, C = x.shape
        ctx.shape = (N, H, W, C)
        if use_native(x):
            return native().avgpool_global(x.contiguous())
        return x.float().mean(dim=(1, 2)).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C = ctx.shape
        if use_native(dy):
            return native().avgpool_global_bwd(dy.contiguous(), H, W)
        return (dy[:, None, None, :] / (H * W)).expand(N, H, W, C).to(dy.dtype)


def global_avg_pool_nhwc(x):
    return _GlobalAvgPoolFn.apply(x)


class _MaxPool2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, stride, pad):
        if use_native(x):
            y, idx = native().maxpool2d_fwd(x.contiguous(), k, stride, pad)
        else:
            xc = x.permute(0, 3, 1, 2).float()
            y, idx = F.max_pool2d(xc, k, stride, pad, return_indices=True)
            y = y.permute(0, 2, 3, 1).contiguous().to(x.dtype)
            idx = idx.permute(0, 2, 3, 1).contiguous()
        ctx.save_for_backward(idx)
        ctx.meta = (x.shape, k, stride, pad, x.is_cuda)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        shape, k, stride, pad, on_gpu = ctx.meta
        if use_native(dy):
            dx = native().maxpool2d_bwd(dy.contiguous(), idx, shape[1], shape[2])
        else:
            # scatter-add (max_unpool2d overwrites ties instead of summing)
            N, H, W, C = shape
            dyc = dy.permute(0, 3, 1, 2).reshape(N, C, -1).float()
            idxc = idx.permute(0, 3, 1, 2).reshape(N, C, -1)
            dxc = torch.zeros(N, C, H * W, dtype=torch.float32)
            dxc.scatter_add_(2, idxc, dyc)
            dx = (
                dxc.reshape(N, C, H, W)
                .permute(0, 2, 3, 1)
                .contiguous()
                .to(dy.dtype)
            )
        return dx, None, None, None


def max_pool2d_nhwc(x, k, stride, pad):
    return _MaxPool2dFn.apply(x, k, stride, pad)


# ---------------------------------------------------------------------------
# LayerNorm / GELU (ViT path)
# ---------------------------------------------------------------------------


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        xs = x.reshape(-1, x.shape[-1])
        if use_native(x, gamma):
            y, mean, rstd = native().layernorm_fwd(xs.contiguous(), gamma, beta, eps)
        else:
            xf = xs.float()
            mean = xf.mean(-1, keepdim=True)
            var = xf.var(-1, unbiased=False, keepdim=True)
            rstd = (var + eps).rsqrt()
            y = ((xf - mean) * rstd * gamma.float() + beta.float()).to(x.dtype)
            mean = mean.squeeze(-1)
            rstd = rstd.squeeze(-1)
        ctx.save_for_backward(x, gamma, mean, rstd)
        return y.reshape_as(x)

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        D = x.shape[-1]
        dys = dy.reshape(-1, D).contiguous()
        xs = x.reshape(-1, D)
        if use_native(dy, gamma):
            dx, dgamma, dbeta = native().layernorm_bwd(
                dys, xs.contiguous(), gamma, mean, rstd
            )
            dgamma = dgamma.to(gamma.dtype)
            dbeta = dbeta.to(gamma.dtype)
        else:
            xf = xs.float()
            dyf = dys.float()
            xhat = (xf - mean[:, None]) * rstd[:, None]
            dgamma = (dyf * xhat).sum(0).to(gamma.dtype)
            dbeta = dyf.sum(0).to(gamma.dtype)
            g = dyf * gamma.float()
            dx = (
                rstd[:, None]
                * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
            ).to(x.dtype)
        return dx.reshape_as(x), dgamma, dbeta, None


def layer_norm(x, gamma, beta, eps=1e-6):
    return _LayerNormFn.apply(x, gamma, beta, eps)


class _GeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        if use_native(x):
            return native().gelu_fwd(x.contiguous())
        return F.gelu(x.float()).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        if use_native(dy):
            return native().gelu_bwd(dy.contiguous(), x)
        xf = x.float().detach().requires_grad_(True)
        with torch.enable_grad():
            y = F.gelu(xf)
        (dx,) = torch.autograd.grad(y, xf, dy.float())
        return dx.to(x.dtype)


def gelu(x):
    return _GeluFn.apply(x)


# ---------------------------------------------------------------------------
# Transformer MLP: Linear -> GELU -> Linear (+ residual), GEMM-epilogue fused
# ---------------------------------------------------------------------------


class _MlpGeluFn(torch.autograd.Function):
    """The MLP on the epilogue kinds of the 256x256 NT kernel
    (``gemm_nt_epi``, ops/csrc/gemm_plain.hip): fc1 writes y = x w1^T + b1 and
    g = gelu(y) from one tile, fc2 adds bias and residual as it stores, and
    fc2's data gradient is multiplied by gelu'(y) as it stores, so no GELU,
    GELU-backward or add pass runs over the activations.  No host reads."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, residual):
        ext = native()
        xs = x.reshape(-1, x.shape[-1]).contiguous()
        w1, w2 = w1.contiguous(), w2.contiguous()
        y, g = ext.gemm_nt_epi(xs, w1, b1, "bias_gelu", None)
        if residual is None:
            out = ext.gemm_nt(g, w2, b2, False, False)
        else:
            res = residual.reshape(-1, w2.shape[0]).contiguous()
            out, _ = ext.gemm_nt_epi(g, w2, b2, "bias_res", res)
        ctx.save_for_backward(xs, y, g, w1, w2)
        ctx.has_res = residual is not None
        return out.reshape(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dout):
        xs, y, g, w1, w2 = ctx.saved_tensors
        ext = native()
        douts = dout.reshape(-1, dout.shape[-1]).contiguous()
        dz, _ = ext.gemm_nt_epi(
            douts, ext.transpose2d(w2), None, "mul_dgelu", y)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ext.gemm_nt(dz, ext.transpose2d(w1), None, False, False)
            dx = dx.reshape(*dout.shape[:-1], w1.shape[1])
        # bias grads ride inside the TN GEMMs (dy is staged anyway)
        dw2, db2 = ext.gemm_tn_bias(douts, g)
        dw1, db1 = ext.gemm_tn_bias(dz, xs)
        dres = dout if ctx.has_res and ctx.needs_input_grad[5] else None
        return (dx, dw1.to(w1.dtype), db1.to(w1.dtype), dw2.to(w2.dtype),
                db2.to(w2.dtype), dres)


def _mlp_fused_ok(x, w1, b1, w2, b2, residual) -> bool:
    # off unless PDT_MLP_FUSED=1: measured slower than the library GEMM plus
    # the separate pass at the ViT-B shapes (profiles/r18_mlp_gelu.md)
    if os.environ.get("PDT_MLP_FUSED", "0") != "1":
        return False
    if b1 is None or b2 is None:
        return False
    ts = [x, w1, b1, w2, b2] + ([] if residual is None else [residual])
    if not use_native(*ts) or any(t.dtype != torch.bfloat16 for t in ts):
        return False
    hidden, c = w1.shape
    c_out = w2.shape[0]
    return (hidden % 256 == 0 and c % 256 == 0 and c_out % 256 == 0
            and w2.shape[1] == hidden and x.shape[-1] == c and x.numel() > 0
            and (residual is None
                 or residual.shape == (*x.shape[:-1], c_out)))


def mlp_gelu(x, w1, b1, w2, b2, residual=None):
    """(residual +) linear(gelu(linear(x, w1, b1)), w2, b2); x (..., C),
    w1 (H, C), w2 (C_out, H).

    With ``PDT_MLP_FUSED=1`` (read per call), bf16 on the GPU with H, C and
    C_out multiples of 256 runs the epilogue-fused GEMMs above; everything
    else (the default, CPU, fp16, fp32, other widths, a missing bias) is
    composed from ``linear`` / ``gelu`` and a plain add, so the function is
    total."""
    if _mlp_fused_ok(x, w1, b1, w2, b2, residual):
        return _MlpGeluFn.apply(x, w1, b1, w2, b2, residual)
    h = linear(gelu(linear(x, w1, b1)), w2, b2)
    return h if residual is None else residual + h


# ---------------------------------------------------------------------------
# Batched GEMM + softmax + attention (ViT path)
# ---------------------------------------------------------------------------


class _BmmNTFn(torch.autograd.Function):
    """C[b,M,N] = A[b,M,K] @ B[b,N,K]^T — both operands K-contiguous."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        if use_native(a, b):
            return native().bmm_nt(a.contiguous(), b.contiguous())
        return torch.einsum("bmk,bnk->bmn", a.float(), b.float()).to(a.dtype)

    @staticmethod
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        dc = dc.contiguous()
        if use_native(dc):
            ext = native()
            da = ext.bmm_nn(dc, b.contiguous())  # dC[b,M,N] @ B[b,N,K]
            db = ext.bmm_tn(dc, a.contiguous())  # dC^T[b,N,M] @ A[b,M,K]
        else:
            da = torch.einsum("bmn,bnk->bmk", dc.float(), b.float()).to(a.dtype)
            db = torch.einsum("bmn,bmk->bnk", dc.float(), a.float()).to(b.dtype)
        return da, db


class _BmmNNFn(torch.autograd.Function):
    """C[b,M,N] = A[b,M,K] @ B[b,K,N] — B N-contiguous."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        if use_native(a, b):
            return native().bmm_nn(a.contiguous(), b.contiguous())
        return torch.einsum("bmk,bkn->bmn", a.float(), b.float()).to(a.dtype)

    @staticmethod
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        dc = dc.contiguous()
        if use_native(dc):
            ext = native()
            da = ext.bmm_nt(dc, b.contiguous())  # dC[b,M,N] @ B^T -> [b,M,K]
            db = ext.bmm_tn(a.contiguous(), dc)  # A^T[b,K,M] @ dC[b,M,N]
        else:
            da = torch.einsum("bmn,bkn->bmk", dc.float(), b.float()).to(a.dtype)
            db = torch.einsum("bmk,bmn->bkn", a.float(), dc.float()).to(b.dtype)
        return da, db


def bmm_nt(a, b):
    return _BmmNTFn.apply(a, b)


def bmm_nn(a, b):
    return _BmmNNFn.apply(a, b)


class _SoftmaxFn(torch.autograd.Function):
    """Row softmax over the last dim, with optional pre-scale."""

    @staticmethod
    def forward(ctx, x, scale):
        xs = x.reshape(-1, x.shape[-1])
        if use_native(x):
            y = native().softmax_fwd(xs.contiguous(), float(scale))
        else:
            y = torch.softmax(xs.float() * scale, dim=-1).to(x.dtype)
        y = y.reshape_as(x)
        ctx.save_for_backward(y)
        ctx.scale = scale
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        D = y.shape[-1]
        dys = dy.reshape(-1, D).contiguous()
        ys = y.reshape(-1, D)
        if use_native(dy):
            dx = native().softmax_bwd(dys, ys.contiguous(), float(ctx.scale))
        else:
            yf, dyf = ys.float(), dys.float()
            dx = (yf * (dyf - (yf * dyf).sum(-1, keepdim=True)) * ctx.scale).to(
                dy.dtype
            )
        return dx.reshape_as(y), None


def softmax(x, scale=1.0):
    return _SoftmaxFn.apply(x, scale)


def _attn_drop_args(x, cid, p):
    """Trailing dropout arguments of attn_fwd / attn_bwd / attn_dropout under
    the current rng state; none at rate 0."""
    if p == 0:
        return ()
    k0, k1 = rng.key()
    return rng.step_scalar(x.device), k0, k1, cid, p


class _AttentionQKVFn(torch.autograd.Function):
    """Fused attention from the PACKED qkv tensor.

    Forward: one kernel (staging from qkv, QK^T, softmax, PV — no q/k/v
    permute kernels), saving only the per-row softmax stats (no S×S P
    materialization).  Backward: flash-style fused kernel (attn_bwd) that
    recomputes P tiles from Q/K + stats and chains the five MFMA products
    per tile pair in LDS — the round-1 composed backward's wide-TN P-grad
    GEMMs, softmax_bwd pass, and P HBM traffic all disappear (VERDICT r1
    item 2).

    p > 0: dropout on the probabilities inside both kernels (the attention
    mask of ops/rng.py).  The forward takes one call id; the backward
    regenerates the mask from it, the step scalar and the key, so nothing is
    stored and nothing may tick in between."""

    @staticmethod
    def forward(ctx, qkv, heads, scale, p):
        ctx.cid = rng.next_call_id() if p > 0 else 0
        out, _, stats = native().attn_fwd(
            qkv, heads, scale, False, *_attn_drop_args(qkv, ctx.cid, p)
        )
        ctx.save_for_backward(qkv, out, stats)
        ctx.heads, ctx.scale, ctx.p = heads, scale, p
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, stats = ctx.saved_tensors
        dqkv = native().attn_bwd(
            qkv, dout.contiguous(), out, stats, ctx.heads, ctx.scale,
            *_attn_drop_args(qkv, ctx.cid, ctx.p)
        )
        return dqkv, None, None, None


class _AttentionQKVComposedFn(torch.autograd.Function):
    """Fused forward + COMPOSED backward (batched MFMA GEMMs on a
    materialized P) — the round-1 path, kept as the numerics reference the
    flash backward is tested against."""

    @staticmethod
    def forward(ctx, qkv, heads, scale):
        out, P, _ = native().attn_fwd(qkv, heads, scale, True)
        ctx.save_for_backward(qkv, P)
        ctx.heads, ctx.scale = heads, scale
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, P = ctx.saved_tensors
        ext = native()
        N, S, D3 = qkv.shape
        h = ctx.heads
        B = N * h
        q, k, v = ext.qkv_unpack(qkv, h)
        do = ext.head_split(dout.contiguous(), h)
        dv = ext.bmm_tn(P, do)                      # P^T @ dO
        dp = ext.bmm_nt(do, v)                      # dO @ V^T
        ds = ext.softmax_bwd(
            dp.reshape(-1, S).contiguous(), P.reshape(-1, S), ctx.scale
        ).reshape(B, S, S)
        dq = ext.bmm_nn(ds, k)                      # dS @ K
        dk = ext.bmm_tn(ds, q)                      # dS^T @ Q
        dqkv = ext.qkv_pack(
            dq.contiguous(), dk.contiguous(), dv.contiguous(), N, h
        )
        return dqkv, None, None


def attention_qkv(qkv, heads, scale, p=0.0, training=True):
    """qkv: [N, S, 3*heads*dh] packed (the qkv Linear output).  p: dropout
    rate on the probabilities; eval mode or p == 0 runs the kernels without
    it, takes no call id and launches nothing else."""
    rng.attn_keep_threshold(p)  # rejects rates outside [0, 1) and (0, 1/256)
    if not training:
        p = 0.0
    return _AttentionQKVFn.apply(qkv, heads, scale, float(p))


def attention_qkv_composed(qkv, heads, scale):
    """Round-1 composed-backward variant (numerics reference for tests)."""
    return _AttentionQKVComposedFn.apply(qkv, heads, scale)


def _attn_dropout_apply(x, cid, p):
    """keep ? x * scale : 0 on [B, S, S] under the attention mask of cid."""
    if use_native(x):
        return native().attn_dropout(x, *_attn_drop_args(x, cid, p))
    # CPU path: the same bits from the same state (ops/rng.py)
    step = int(rng.step_scalar(x.device).item())
    keep = rng.attn_keep_mask(x.shape[0], x.shape[1], p, cid, step)
    zero = torch.zeros((), dtype=torch.float32)
    return torch.where(keep, x.float() * rng.attn_keep_scale(p), zero).to(
        x.dtype
    )


class _AttnDropoutFn(torch.autograd.Function):
    """Dropout on materialised probabilities [B, S, S] with the mask the fused
    attention kernels draw; backward is the same op on the gradient."""

    @staticmethod
    def forward(ctx, pm, p):
        ctx.cid, ctx.p = rng.next_call_id(), p
        return _attn_dropout_apply(pm.contiguous(), ctx.cid, p)

    @staticmethod
    def backward(ctx, dy):
        return _attn_dropout_apply(dy.contiguous(), ctx.cid, ctx.p), None


def attention(q, k, v, scale, p=0.0, training=True):
    """Batched attention out = dropout(softmax(Q K^T * scale), p) V.

    q,k,v: (B, S, d) with d contiguous.  Composed from the MFMA bmm kernels
    + the fused softmax kernel; the S x S score matrix is materialized
    (fine at ViT sequence lengths; ``attention_qkv`` is the fused route).
    Dropout draws the mask of ``attention_qkv``, so both routes drop the same
    elements from the same rng state.
    """
    rng.attn_keep_threshold(p)  # rejects rates outside [0, 1) and (0, 1/256)
    pm = softmax(bmm_nt(q, k), scale)
    if training and p > 0:
        pm = _AttnDropoutFn.apply(pm, float(p))
    return bmm_nn(pm, v)


# ---------------------------------------------------------------------------
# Shifted-window attention (Swin): 7x7 windows, relative-position bias, mask
# ---------------------------------------------------------------------------

WINDOW = 7
_WIN_HEAD_DIM = 32  # what the fused kernels are built for


class _WindowAttentionFn(torch.autograd.Function):
    """Fused window attention from the PACKED qkv map [N, H, W, 3*heads*32]
    (ops/csrc/window_attention.hip).  Shift, window partition, head split and
    their inverses are address arithmetic inside the two kernels; scores,
    probabilities and the mask never exist in memory, and the backward
    recomputes the probabilities, so only the inputs are saved."""

    @staticmethod
    def forward(ctx, qkv, bias_table, heads, shift, scale):
        qkv = qkv.contiguous()
        ctx.save_for_backward(qkv, bias_table)
        ctx.args = (heads, shift, scale)
        return native().win_attn_fwd(qkv, bias_table, *ctx.args)

    @staticmethod
    def backward(ctx, dout):
        qkv, bias_table = ctx.saved_tensors
        dqkv, dbias = native().win_attn_bwd(
            dout.contiguous(), qkv, bias_table, *ctx.args
        )
        return dqkv, dbias.to(bias_table.dtype), None, None, None


def _window_bias_mask(bias_table, H, W, heads, shift):
    """The additive term of the scores, [nW or 1, heads, 49, 49]: the table's
    row (dy+6)*13 + (dx+6) for query - key offset (dy, dx), and -100 between
    tokens of different regions of the shifted frame."""
    dev = bias_table.device
    t = torch.arange(WINDOW * WINDOW, device=dev)
    ti, tj = t // WINDOW, t % WINDOW
    rel = (ti[:, None] - ti[None, :] + 6) * 13 + (tj[:, None] - tj[None, :] + 6)
    add = bias_table[rel.reshape(-1)].reshape(49, 49, heads).permute(2, 0, 1)
    add = add.unsqueeze(0)
    if shift == 0:
        return add

    def region(size, tok):
        # 0, 1 or 2 for the shifted-frame coordinate 7*w + tok of every
        # (window, token) along one axis
        c = torch.arange(size // WINDOW, device=dev)[:, None] * WINDOW + tok
        return (c >= size - WINDOW).long() + (c >= size - shift).long()

    reg = 3 * region(H, ti)[:, None, :] + region(W, tj)[None, :, :]
    reg = reg.reshape(-1, 49)                            # [nh*nw, 49]
    mask = (reg[:, :, None] != reg[:, None, :]).to(add.dtype) * -100.0
    return add + mask[:, None]


def _window_attention_composed(qkv, bias_table, heads, shift, scale):
    """The same function from torch.roll / reshape copies and the batched
    GEMM + softmax ops, with scores and probabilities materialised."""
    N, H, W, C3 = qkv.shape
    dh = C3 // (3 * heads)
    nh, nw = H // WINDOW, W // WINDOW
    x = torch.roll(qkv, (-shift, -shift), (1, 2)) if shift else qkv
    x = x.reshape(N, nh, WINDOW, nw, WINDOW, 3, heads, dh)
    x = x.permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, -1, 49, dh)
    q, k, v = x[0].contiguous(), x[1].contiguous(), x[2].contiguous()
    add = _window_bias_mask(bias_table.to(qkv.dtype), H, W, heads, shift)
    s = bmm_nt(q, k).reshape(N, nh * nw, heads, 49, 49) * scale + add
    o = bmm_nn(softmax(s.reshape(-1, 49, 49)), v)
    o = o.reshape(N, nh, nw, heads, WINDOW, WINDOW, dh)
    o = o.permute(0, 1, 4, 2, 5, 3, 6).reshape(N, H, W, heads * dh)
    return torch.roll(o, (shift, shift), (1, 2)) if shift else o


def window_attention(qkv, bias_table, heads, shift, scale):
    """Swin's (shifted-)window multi-head attention on an NHWC map.

    qkv: [N, H, W, 3*heads*32] packed ``[3][heads][32]`` (the qkv Linear's
    output); bias_table: [169, heads]; returns [N, H, W, heads*32] in the image
    layout.  Window 7x7, so H and W must be multiples of 7 (no padding), and
    0 <= shift < 7.  bf16/fp16 on the GPU runs the fused kernels; fp32 and the
    CPU take the composed route."""
    if qkv.dim() != 4 or qkv.shape[3] % (3 * heads):
        raise ValueError(
            "window_attention: qkv must be [N, H, W, 3*heads*dh], got "
            f"{tuple(qkv.shape)} for {heads} heads")
    dh = qkv.shape[3] // (3 * heads)
    if dh != _WIN_HEAD_DIM:
        raise ValueError(
            f"window_attention: the head dim must be {_WIN_HEAD_DIM}, got {dh}")
    if qkv.shape[1] % WINDOW or qkv.shape[2] % WINDOW:
        raise ValueError(
            "window_attention: H and W must be multiples of the window size "
            f"{WINDOW} (no padding), got {qkv.shape[1]}x{qkv.shape[2]}")
    if not 0 <= shift < WINDOW:
        raise ValueError(
            f"window_attention: shift must be in [0, {WINDOW}), got {shift}")
    if tuple(bias_table.shape) != (169, heads):
        raise ValueError(
            "window_attention: bias_table must be [169, heads], got "
            f"{tuple(bias_table.shape)}")
    if use_native(qkv) and qkv.dtype in (torch.bfloat16, torch.float16):
        return _WindowAttentionFn.apply(
            qkv, bias_table, heads, int(shift), float(scale))
    return _window_attention_composed(qkv, bias_table, heads, int(shift), scale)


# ---------------------------------------------------------------------------
# Dropout / stochastic depth (+ fused residual add), Philox in-kernel
# ---------------------------------------------------------------------------


def _dropout_apply(x, res, cid_e, cid_r, p, p_row, inner):
    """(res or 0) + x * elem mask * row mask under the current rng state.
    p == 0 / p_row == 0 switches that mask off; x (and res) contiguous."""
    if use_native(x, res):
        k0, k1 = rng.key()
        return native().dropout_fwd(
            x, res, None, rng.step_scalar(x.device), k0, k1, cid_e, cid_r,
            float(p), float(p_row), inner,
        )
    # CPU path: the same bits from the same state (ops/rng.py)
    step = int(rng.step_scalar(x.device).item())
    n = x.numel()
    t = x.float().reshape(-1)
    zero = torch.zeros((), dtype=torch.float32, device=t.device)
    if p > 0:
        keep = rng.keep_mask(n, p, cid_e, step).to(t.device)
        t = torch.where(keep, t * rng.keep_scale(p), zero)
    if p_row > 0:
        rows = n // inner if n else 0
        keep = rng.keep_mask(rows, p_row, cid_r, step)
        keep = keep.repeat_interleave(inner).to(t.device)
        t = torch.where(keep, t * rng.keep_scale(p_row), zero)
    if res is not None:
        t = res.float().reshape(-1) + t
    return t.to(x.dtype).reshape(x.shape)


class _DropoutAddFn(torch.autograd.Function):
    """out = (res or 0) + x * keep_elem * s_elem * keep_row * s_row.

    No mask is stored: backward is the same kernel on dy with the same call
    ids, rates and step scalar (nothing ticks between forward and backward),
    and the residual's gradient is dy itself."""

    @staticmethod
    def forward(ctx, x, res, p, p_row):
        x = x.contiguous()
        if res is not None:
            res = res.contiguous()
        # one call id per mask, so the two draws never share a word
        ctx.cid_e = rng.next_call_id() if p > 0 else 0
        ctx.cid_r = rng.next_call_id() if p_row > 0 else 0
        ctx.p, ctx.p_row = p, p_row
        ctx.inner = x.numel() // x.shape[0] if x.numel() else 1
        ctx.has_res = res is not None
        return _dropout_apply(x, res, ctx.cid_e, ctx.cid_r, p, p_row, ctx.inner)

    @staticmethod
    def backward(ctx, dy):
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _dropout_apply(dy.contiguous(), None, ctx.cid_e, ctx.cid_r,
                                ctx.p, ctx.p_row, ctx.inner)
        dres = dy if ctx.has_res and ctx.needs_input_grad[1] else None
        return dx, dres, None, None


def _check_rate(p, what):
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{what} rate must be in [0, 1), got {p}")


def dropout(x, p, training=True):
    """Elementwise dropout.  Eval mode or p == 0 returns x, launches nothing
    and takes no call id."""
    _check_rate(p, "dropout")
    if not training or p == 0:
        return x
    return _DropoutAddFn.apply(x, None, float(p), 0.0)


def drop_path(x, p, training=True):
    """Stochastic depth: one draw per index of dim 0."""
    _check_rate(p, "drop_path")
    if not training or p == 0:
        return x
    return _DropoutAddFn.apply(x, None, 0.0, float(p))


def dropout_add(x, res, p, p_path, training=True):
    """res + drop_path(dropout(x, p), p_path) in one pass over the data."""
    _check_rate(p, "dropout")
    _check_rate(p_path, "drop_path")
    if not training or (p == 0 and p_path == 0):
        return res + x
    if x.shape != res.shape or x.dtype != res.dtype:
        raise ValueError("dropout_add: x and res must match in shape and dtype")
    return _DropoutAddFn.apply(x, res, float(p), float(p_path))


# ---------------------------------------------------------------------------
# Multi-tensor optimizer / grad utilities (used by optim + engine)
# ---------------------------------------------------------------------------


def grad_l2_norm(grads) -> torch.Tensor:
    """Global L2 norm over a list of grads (reference ddp.py:238-239)."""
    grads = [g for g in grads if g is not None]
    if not grads:
        return torch.zeros(())
    if use_native(*grads):
        sq = native().l2norm_sq(list(grads))
        return sq.sqrt()
    return torch.sqrt(sum(g.float().pow(2).sum() for g in grads))


def scale_grads_(grads, scale: float) -> None:
    grads = [g for g in grads if g is not None]
    if not grads:
        return
    if use_native(*grads):
        native().scale_(list(grads), float(scale))
    else:
        for g in grads:
            g.mul_(scale)
