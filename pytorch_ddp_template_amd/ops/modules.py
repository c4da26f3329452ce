"""nn.Module wrappers over the HIP-backed functional ops.

These mirror the torch.nn API surface (parameter names, state_dict layout)
so checkpoints look conventional, but dispatch to the CDNA4 kernels.
Conv/BN modules are NHWC (see ops/functional.py).
"""

from __future__ import annotations

import math

import torch
from torch import nn

from . import functional as X
from . import rng


class Linear(nn.Module):
    def __init__(self, in_features, out_features, bias=True, act=None):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.act = act
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1.0 / math.sqrt(self.in_features)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x):
        return X.linear(x, self.weight, self.bias, self.act)

    def extra_repr(self):
        return (
            f"in_features={self.in_features}, out_features={self.out_features},"
            f" bias={self.bias is not None}, act={self.act}"
        )


class ReLU(nn.Module):
    def forward(self, x):
        return X.relu(x)


class GELU(nn.Module):
    def forward(self, x):
        return X.gelu(x)


class Dropout(nn.Module):
    """Elementwise dropout with the mask drawn in the kernel (ops/rng.py)."""

    def __init__(self, p=0.5):
        super().__init__()
        self.p = float(p)

    def forward(self, x):
        return X.dropout(x, self.p, self.training)

    def extra_repr(self):
        return f"p={self.p}"


class DropPath(nn.Module):
    """Stochastic depth: drops whole samples (indices of dim 0)."""

    def __init__(self, p=0.0):
        super().__init__()
        self.p = float(p)

    def forward(self, x):
        return X.drop_path(x, self.p, self.training)

    def extra_repr(self):
        return f"p={self.p}"


class Conv2dNHWC(nn.Module):
    """Conv2d on (N, H, W, C) tensors; weight stored (K, R, S, C / groups).
    groups: 1, or in_ch == out_ch for a depthwise conv."""

    def __init__(
        self, in_ch, out_ch, kernel_size, stride=1, padding=0, bias=False,
        act=None, groups=1
    ):
        super().__init__()
        k = (
            (kernel_size, kernel_size)
            if isinstance(kernel_size, int)
            else tuple(kernel_size)
        )
        if in_ch % groups or out_ch % groups:
            raise ValueError("Conv2dNHWC: groups must divide in_ch and out_ch")
        self.in_ch, self.out_ch, self.groups = in_ch, out_ch, groups
        self.kernel_size, self.stride, self.padding = k, stride, padding
        self.act = act
        self.weight = nn.Parameter(
            torch.empty(out_ch, k[0], k[1], in_ch // groups))
        self.bias = nn.Parameter(torch.empty(out_ch)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        fan_in = (self.in_ch // self.groups) * self.kernel_size[0] \
            * self.kernel_size[1]
        nn.init.normal_(self.weight, 0.0, math.sqrt(2.0 / fan_in))
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x):
        return X.conv2d_nhwc(
            x, self.weight, self.bias, self.stride, self.padding, self.act,
            self.groups
        )

    def extra_repr(self):
        return (
            f"{self.in_ch}, {self.out_ch}, kernel_size={self.kernel_size},"
            f" stride={self.stride}, padding={self.padding}, act={self.act}"
            + (f", groups={self.groups}" if self.groups != 1 else "")
        )


class BatchNorm2dNHWC(nn.Module):
    def __init__(self, num_features, eps=1e-5, momentum=0.1, act=None):
        super().__init__()
        self.num_features = num_features
        self.eps = eps
        self.momentum = momentum
        self.act = act
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        # tracked count lives host-side (a GPU scalar += here cost a kernel
        # launch per BN layer per step); it enters state_dict via the
        # _save/_load hooks below so checkpoints still carry it.
        self._batches_tracked = 0
        # this BN+ReLU's output feeds a wired fused block and nothing else
        # (functional._BatchNorm2dFn); off unless ResNet wires the stem
        self._out_to_block = False

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        destination[prefix + "num_batches_tracked"] = torch.tensor(
            self._batches_tracked, dtype=torch.long
        )

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        key = prefix + "num_batches_tracked"
        if key in state_dict:
            self._batches_tracked = int(state_dict.pop(key))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _apply(self, fn, recurse=True):
        # Running stats stay fp32 regardless of model dtype: the BN kernels
        # accumulate and update them in fp32 (model.to(bf16) must not
        # downcast them).
        super()._apply(fn, recurse)
        self.running_mean.data = self.running_mean.data.float()
        self.running_var.data = self.running_var.data.float()
        return self

    def forward(self, x):
        if self.training:
            self._batches_tracked += 1
        return X.batch_norm2d_nhwc(
            x,
            self.weight,
            self.bias,
            self.running_mean,
            self.running_var,
            self.training,
            self.momentum,
            self.eps,
            self.act,
            self._out_to_block,
        )

    def extra_repr(self):
        return f"{self.num_features}, eps={self.eps}, momentum={self.momentum}, act={self.act}"


class LayerNorm(nn.Module):
    def __init__(self, dim, eps=1e-6):
        super().__init__()
        self.dim = dim
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))

    def forward(self, x):
        return X.layer_norm(x, self.weight, self.bias, self.eps)


class WindowAttention(nn.Module):
    """Swin's window multi-head attention on an NHWC map [N, H, W, dim]: 7x7
    windows, cyclically shifted by ``shift`` pixels, with a learned
    relative-position bias per head (``X.window_attention``)."""

    def __init__(self, dim, heads, shift=0):
        super().__init__()
        if dim % heads:
            raise ValueError("WindowAttention: heads must divide dim")
        self.dim, self.heads, self.shift = dim, heads, int(shift)
        self.qkv = Linear(dim, 3 * dim)
        self.proj = Linear(dim, dim)
        self.relative_position_bias_table = nn.Parameter(
            torch.zeros((2 * X.WINDOW - 1) ** 2, heads))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)

    def forward(self, x):
        out = X.window_attention(
            self.qkv(x), self.relative_position_bias_table, self.heads,
            self.shift, (self.dim // self.heads) ** -0.5)
        return self.proj(out)

    def extra_repr(self):
        return f"dim={self.dim}, heads={self.heads}, shift={self.shift}"


class GlobalAvgPoolNHWC(nn.Module):
    def forward(self, x):
        return X.global_avg_pool_nhwc(x)


class MaxPool2dNHWC(nn.Module):
    def __init__(self, kernel_size, stride, padding=0):
        super().__init__()
        self.kernel_size, self.stride, self.padding = kernel_size, stride, padding

    def forward(self, x):
        return X.max_pool2d_nhwc(x, self.kernel_size, self.stride, self.padding)


class MSELoss(nn.Module):
    """The reference's criterion (ddp.py:164)."""

    def forward(self, pred, target):
        return X.mse_loss(pred, target)


class CrossEntropyLoss(nn.Module):
    """Fused log-softmax + NLL, mean reduction.

    label_smoothing / mix (a :class:`BatchMix`) switch to the soft-target
    kernels, in train mode only; eval mode and the argument-free form are the
    hard-label loss."""

    def __init__(self, label_smoothing=0.0, mix=None):
        super().__init__()
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(
                f"label_smoothing must be in [0, 1), got {label_smoothing}")
        self.label_smoothing = float(label_smoothing)
        self.mix = mix

    def forward(self, logits, target):
        if not self.training:
            return X.cross_entropy(logits, target)
        return X.cross_entropy(logits, target, self.label_smoothing, self.mix)

    def extra_repr(self):
        return f"label_smoothing={self.label_smoothing}, mix={self.mix}"


class BatchMix:
    """Mixup / cutmix of an image batch with its flip (sample i with B-1-i).

    One draw per call: lambda ~ Beta(alpha, alpha), the choice between the two
    modes and the cutmix box all come from the counter-based generator of
    ``ops/rng.py`` and are drawn ON THE DEVICE into the params record, which
    the mix kernel and the loss (``CrossEntropyLoss(mix=self)``) read there.  A
    captured step therefore mixes differently on every replay.  Not an
    nn.Module: it holds no weights and nothing for a checkpoint.

    mixup_alpha / cutmix_alpha: 0 switches that mode off; at most 1 (the
    wave-wide Beta sampler's limit).  prob: chance that a batch is mixed at
    all; switch_prob: chance of cutmix when both modes are on."""

    def __init__(self, mixup_alpha, cutmix_alpha, prob=1.0, switch_prob=0.5):
        rng.check_mix_args(mixup_alpha, cutmix_alpha, prob, switch_prob)
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        self._params = {}

    def params(self, device) -> torch.Tensor:
        """The device's record (8 four-byte slots, see ``rng.mix_record``),
        created on first use as "not applied" and never reallocated."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._params.get(device)
        if t is None:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(
                    "BatchMix.params: the params record of a device must "
                    "exist before a stream capture begins (run one eager "
                    "step, or call params(device) first)"
                )
            t = self._params[device] = rng.mix_record().to(device)
        return t

    def apply_(self, x):
        """Draw this call's parameters and mix x in place; returns x."""
        if x.dim() != 4:
            raise ValueError("BatchMix.apply_: x must be a 4-D image batch")
        nchw = x.shape[1] == 3 and x.shape[-1] != 3  # the models' rule
        H, W = (x.shape[2], x.shape[3]) if nchw else (x.shape[1], x.shape[2])
        params = self.params(x.device)
        step = rng.step_scalar(x.device)
        cid = rng.next_call_id()
        args = (H, W, self.mixup_alpha, self.cutmix_alpha, self.prob,
                self.switch_prob)
        if X.use_native(x):
            k0, k1 = rng.key()
            X.native().mix_draw(params, step, k0, k1, cid, *args)
        else:
            d = rng.mix_draw(*args, cid, int(step.item()))
            params.copy_(rng.mix_record(
                d["lam"], d["a"], (d["y0"], d["y1"], d["x0"], d["x1"]),
                d["mode"], d["raw"]))
        return X.batch_mix_(x, params)

    def __repr__(self):
        return (f"BatchMix(mixup_alpha={self.mixup_alpha}, cutmix_alpha="
                f"{self.cutmix_alpha}, prob={self.prob}, switch_prob="
                f"{self.switch_prob})")
