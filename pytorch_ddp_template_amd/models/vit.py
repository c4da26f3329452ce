"""ViT-B/16 on the framework's HIP-backed ops (BASELINE.json config 5).

Attention runs in the fused flash-style kernel (``attention_qkv``: q/k/v
staged straight from the packed qkv GEMM output, K/V tiled, no score matrix
in memory) whenever the head size is 64 and the dtype is bf16/fp16 on the
GPU; every other case (fp32, other head sizes, the CPU path) is composed
from the batched GEMM primitives (``bmm_nt`` / ``bmm_nn``) plus the fused
row-softmax kernel, with the score matrix materialized.

Patch embedding is a Linear over unfolded 16x16x3 patches (= 768-dim
vectors), which on NHWC input is a pure reshape + one GEMM — no conv needed.

Regularisation (``dropout`` / ``drop_path``, both 0 by default): dropout
after the position-embedding add, on the attention projection output, after
the MLP's GELU and on the MLP output; stochastic depth on both residual
branches of block ``i`` at rate ``drop_path * i / (depth - 1)``.  Each
residual is ONE ``dropout_add`` kernel (element mask, per-sample mask and the
add), masks come from the counter-based generator in ``ops/rng.py`` and are
never stored.  With both rates 0, and in eval mode, the forward runs exactly
the ops of the unregularised model; the modules hold no extra state, so
``state_dict`` keys do not depend on the rates.  Not covered: dropout on the
attention probabilities (it belongs inside the attention kernel), fusing the
post-GELU dropout into the GELU kernel, label smoothing.
"""

from __future__ import annotations

import math

import torch
from torch import nn

from ..ops import GELU, LayerNorm, Linear
from ..ops.functional import attention, attention_qkv, dropout, dropout_add
from ..ops.native import native_available


class MultiHeadAttention(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        assert dim % heads == 0
        self.dim, self.heads = dim, heads
        self.qkv = Linear(dim, 3 * dim)
        self.proj = Linear(dim, dim)

    def forward(self, x):
        # x: (N, S, D)
        N, S, D = x.shape
        h, dh = self.heads, D // self.heads
        qkv = self.qkv(x)  # (N, S, 3D)
        # the flash forward/backward tile K/V, so S is uncapped (the old
        # S<=224 limit belonged to the P-materializing two-pass kernel;
        # fused-vs-composed grads are tested at S=320)
        if (
            x.is_cuda and dh == 64
            and x.dtype in (torch.bfloat16, torch.float16)
            and native_available()
        ):
            # fused kernel: stages q/k/v straight from the packed qkv
            out = attention_qkv(qkv.contiguous(), h, 1.0 / math.sqrt(dh))
            return self.proj(out)
        qkv = qkv.reshape(N, S, 3, h, dh).permute(2, 0, 3, 1, 4)
        q, k, v = (t.reshape(N * h, S, dh).contiguous() for t in qkv)
        out = attention(q, k, v, 1.0 / math.sqrt(dh))  # (N*h, S, dh)
        out = out.reshape(N, h, S, dh).permute(0, 2, 1, 3).reshape(N, S, D)
        return self.proj(out)


class Block(nn.Module):
    def __init__(self, dim, heads, mlp_ratio=4, dropout=0.0, drop_path=0.0):
        super().__init__()
        self.p, self.p_path = float(dropout), float(drop_path)
        self.norm1 = LayerNorm(dim)
        self.attn = MultiHeadAttention(dim, heads)
        self.norm2 = LayerNorm(dim)
        self.mlp = nn.Sequential(
            Linear(dim, dim * mlp_ratio),
            GELU(),
            Linear(dim * mlp_ratio, dim),
        )

    def forward(self, x):
        if not self.training or (self.p == 0 and self.p_path == 0):
            x = x + self.attn(self.norm1(x))
            x = x + self.mlp(self.norm2(x))
            return x
        # mlp's members are called one by one (the Sequential keeps its
        # state_dict keys); each residual is one dropout_add
        x = dropout_add(self.attn(self.norm1(x)), x, self.p, self.p_path, True)
        h = self.mlp[1](self.mlp[0](self.norm2(x)))
        h = self.mlp[2](dropout(h, self.p, True))
        return dropout_add(h, x, self.p, self.p_path, True)


class ViT(nn.Module):
    def __init__(
        self,
        image_size=224,
        patch_size=16,
        dim=768,
        depth=12,
        heads=12,
        mlp_ratio=4,
        num_classes=1000,
        in_ch=3,
        dropout=0.0,
        drop_path=0.0,
    ):
        super().__init__()
        assert image_size % patch_size == 0
        self.p = float(dropout)
        self.patch_size = patch_size
        self.grid = image_size // patch_size
        n_patches = self.grid * self.grid
        patch_dim = patch_size * patch_size * in_ch
        self.patch_embed = Linear(patch_dim, dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, n_patches + 1, dim) )
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.trunc_normal_(self.cls_token, std=0.02)
        # stochastic depth grows linearly from 0 (first block) to drop_path
        self.blocks = nn.Sequential(*[
            Block(dim, heads, mlp_ratio, dropout,
                  drop_path * i / max(depth - 1, 1))
            for i in range(depth)
        ])
        self.norm = LayerNorm(dim)
        self.head = Linear(dim, num_classes)

    def no_weight_decay(self):
        """Parameter names that optim.param_groups_no_decay keeps out of
        weight decay in addition to the ndim <= 1 ones."""
        return {"cls_token", "pos_embed"}

    def _patchify(self, x):
        # NHWC (N, H, W, C) -> (N, n_patches, P*P*C)
        N, H, W, C = x.shape
        P, G = self.patch_size, self.grid
        x = x.reshape(N, G, P, G, P, C).permute(0, 1, 3, 2, 4, 5)
        return x.reshape(N, G * G, P * P * C)

    def forward(self, x):
        if x.dim() == 4 and x.shape[1] == 3 and x.shape[-1] != 3:
            x = x.permute(0, 2, 3, 1).contiguous()
        x = self.patch_embed(self._patchify(x))
        cls = self.cls_token.to(x.dtype).expand(x.shape[0], -1, -1)
        x = torch.cat([cls, x], dim=1) + self.pos_embed.to(x.dtype)
        x = dropout(x, self.p, self.training)
        x = self.blocks(x)
        x = self.norm(x)
        return self.head(x[:, 0])


def vit_b16(num_classes=1000, image_size=224, dropout=0.0, drop_path=0.0):
    return ViT(image_size=image_size, num_classes=num_classes,
               dropout=dropout, drop_path=drop_path)
