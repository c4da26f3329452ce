"""Swin Transformer on the framework's HIP-backed ops, activations NHWC.

Patch embedding: Linear over unfolded 4x4x3 patches (reshape + one GEMM, as in
``vit.py``) + LayerNorm.  Stages of blocks with a patch merging between them
(2x2 concat -> LayerNorm(4C) -> Linear(4C, 2C, no bias)).  Block: LayerNorm ->
window attention -> residual, LayerNorm -> Linear(C, 4C) -> GELU ->
Linear(4C, C) -> residual.  Blocks alternate shift 0 and 3; a map that is a
single 7x7 window is never shifted.  Head: LayerNorm -> global average pool ->
Linear.  LayerNorm eps is 1e-5, Swin's value.

The attention runs in ``ops/csrc/window_attention.hip`` (bf16/fp16 on the
GPU): the activations stay [N, H, W, C] from end to end, and the cyclic shift,
the window partition, the head split and their inverses are address arithmetic
inside that kernel, so none of them is ever a copy.

``drop_path``: stochastic depth at rate ``drop_path * i / (blocks - 1)`` for
block ``i`` over ALL blocks, as in ``vit.py`` / ``convnext.py``; in training
with a nonzero rate each residual is one ``dropout_add`` kernel, otherwise a
plain add.  The modules hold no extra state for it, so ``state_dict`` keys do
not depend on the rate.

Not covered: window sizes other than 7; head dims other than 32; H / W that
are not multiples of 7 (no padding); dropout on the attention probabilities;
a fused patch-merging gather (the 2x2 concat is a torch reshape / permute
copy); Swin-S/B/L presets.
"""

from __future__ import annotations

from torch import nn

from ..ops import GELU, GlobalAvgPoolNHWC, LayerNorm, Linear, WindowAttention
from ..ops.functional import WINDOW, dropout_add, mlp_gelu

_EPS = 1e-5


class Block(nn.Module):
    def __init__(self, dim, heads, shift, mlp_ratio=4, drop_path=0.0):
        super().__init__()
        self.p_path = float(drop_path)
        self.norm1 = LayerNorm(dim, _EPS)
        self.attn = WindowAttention(dim, heads, shift)
        self.norm2 = LayerNorm(dim, _EPS)
        self.mlp = nn.Sequential(
            Linear(dim, dim * mlp_ratio),
            GELU(),
            Linear(dim * mlp_ratio, dim),
        )

    def _residual(self, h, x):
        if self.training and self.p_path > 0:
            return dropout_add(h, x, 0.0, self.p_path, True)
        return x + h

    def forward(self, x):
        x = self._residual(self.attn(self.norm1(x)), x)
        # one mlp_gelu call on the Sequential's parameters; the plain add
        # goes into it (fc2's epilogue where the width is eligible)
        fc1, fc2 = self.mlp[0], self.mlp[2]
        path = self.training and self.p_path > 0
        h = mlp_gelu(self.norm2(x), fc1.weight, fc1.bias, fc2.weight,
                     fc2.bias, None if path else x)
        return dropout_add(h, x, 0.0, self.p_path, True) if path else h


class PatchMerging(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm = LayerNorm(4 * dim, _EPS)
        self.reduction = Linear(4 * dim, 2 * dim, bias=False)

    def forward(self, x):
        # [N, H, W, C] -> [N, H/2, W/2, 4C], channels ordered as Swin's concat
        # of (0,0), (1,0), (0,1), (1,1)
        N, H, W, C = x.shape
        x = x.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 4, 2, 5)
        return self.reduction(self.norm(x.reshape(N, H // 2, W // 2, 4 * C)))


class SwinTransformer(nn.Module):
    def __init__(self, image_size=224, patch_size=4, dims=(96, 192, 384, 768),
                 depths=(2, 2, 6, 2), heads=(3, 6, 12, 24), mlp_ratio=4,
                 num_classes=1000, drop_path=0.0, in_ch=3):
        super().__init__()
        assert len(dims) == len(depths) == len(heads)
        self.patch_size = patch_size
        grid = image_size // patch_size
        if image_size % patch_size or grid % (WINDOW << (len(dims) - 1)):
            raise ValueError(
                f"SwinTransformer: a {image_size}-pixel image in {patch_size}-"
                f"pixel patches is not a whole number of {WINDOW}x{WINDOW} "
                f"windows at each of {len(dims)} stages")
        self.patch_embed = Linear(patch_size * patch_size * in_ch, dims[0])
        self.patch_norm = LayerNorm(dims[0], _EPS)
        total, k = sum(depths), 0
        self.stages = nn.ModuleList()
        self.downsample = nn.ModuleList()
        for s, (dim, depth, h) in enumerate(zip(dims, depths, heads)):
            if s > 0:
                assert dim == 2 * dims[s - 1]
                self.downsample.append(PatchMerging(dims[s - 1]))
            one_window = (grid >> s) == WINDOW
            self.stages.append(nn.Sequential(*[
                Block(dim, h, 0 if (j % 2 == 0 or one_window) else WINDOW // 2,
                      mlp_ratio, drop_path * (k + j) / max(total - 1, 1))
                for j in range(depth)
            ]))
            k += depth
        self.norm = LayerNorm(dims[-1], _EPS)
        self.pool = GlobalAvgPoolNHWC()
        self.head = Linear(dims[-1], num_classes)

    def no_weight_decay(self):
        """The bias tables, in addition to the ndim <= 1 parameters."""
        return {n for n, _ in self.named_parameters()
                if n.endswith("relative_position_bias_table")}

    def _patchify(self, x):
        # NHWC (N, H, W, C) -> (N, H/P, W/P, P*P*C)
        N, H, W, C = x.shape
        P = self.patch_size
        x = x.reshape(N, H // P, P, W // P, P, C).permute(0, 1, 3, 2, 4, 5)
        return x.reshape(N, H // P, W // P, P * P * C)

    def forward(self, x):
        if x.dim() == 4 and x.shape[1] == 3 and x.shape[-1] != 3:
            x = x.permute(0, 2, 3, 1).contiguous()
        x = self.patch_norm(self.patch_embed(self._patchify(x)))
        for s, stage in enumerate(self.stages):
            if s > 0:
                x = self.downsample[s - 1](x)
            x = stage(x)
        return self.head(self.pool(self.norm(x)))


def swin_tiny(num_classes=1000, drop_path=0.0, image_size=224):
    return SwinTransformer(image_size, 4, (96, 192, 384, 768), (2, 2, 6, 2),
                           (3, 6, 12, 24), 4, num_classes, drop_path)
