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

from . import rng
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


def conv2d_nhwc(x, w, b=None, stride=1, pad=0, act=None):
    return _Conv2dFn.apply(x, w, b, stride, pad, act)


# ---------------------------------------------------------------------------
# BatchNorm2d NHWC (optionally fused ReLU)
# ---------------------------------------------------------------------------


class _BatchNorm2dFn(torch.autograd.Function):
    @staticmethod
    def forward(
        ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, act
    ):
        C = x.shape[-1]
        xs = x.reshape(-1, C)
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
            dx, dgamma, dbeta = ext.bn_bwd(
                dys, xs.contiguous(), gamma, mean, rstd, yr
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
):
    return _BatchNorm2dFn.apply(
        x, gamma, beta, running_mean, running_var, training, momentum, eps, act
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


def cross_entropy(logits, target):
    return _CrossEntropyFn.apply(logits, target)


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


class _AttentionQKVFn(torch.autograd.Function):
    """Fused attention from the PACKED qkv tensor.

    Forward: one kernel (staging from qkv, QK^T, softmax, PV — no q/k/v
    permute kernels), saving only the per-row softmax stats (no S×S P
    materialization).  Backward: flash-style fused kernel (attn_bwd) that
    recomputes P tiles from Q/K + stats and chains the five MFMA products
    per tile pair in LDS — the round-1 composed backward's wide-TN P-grad
    GEMMs, softmax_bwd pass, and P HBM traffic all disappear (VERDICT r1
    item 2)."""

    @staticmethod
    def forward(ctx, qkv, heads, scale):
        out, _, stats = native().attn_fwd(qkv, heads, scale, False)
        ctx.save_for_backward(qkv, out, stats)
        ctx.heads, ctx.scale = heads, scale
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, stats = ctx.saved_tensors
        dqkv = native().attn_bwd(
            qkv, dout.contiguous(), out, stats, ctx.heads, ctx.scale
        )
        return dqkv, None, None


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


def attention_qkv(qkv, heads, scale):
    """qkv: [N, S, 3*heads*dh] packed (the qkv Linear output)."""
    return _AttentionQKVFn.apply(qkv, heads, scale)


def attention_qkv_composed(qkv, heads, scale):
    """Round-1 composed-backward variant (numerics reference for tests)."""
    return _AttentionQKVComposedFn.apply(qkv, heads, scale)


def attention(q, k, v, scale):
    """Batched attention out = softmax(Q K^T * scale) V.

    q,k,v: (B, S, d) with d contiguous.  Composed from the MFMA bmm kernels
    + the fused softmax kernel; the S x S score matrix is materialized
    (fine at ViT sequence lengths; flash-style fusion is a later rung).
    """
    p = softmax(bmm_nt(q, k), scale)
    return bmm_nn(p, v)


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
