"""ConvNeXt on the framework's HIP-backed ops, activations NHWC throughout.

Stem: 4x4 stride-4 conv + LayerNorm.  Four stages of blocks, a LayerNorm and
a 2x2 stride-2 conv between them.  Block: depthwise 7x7 (pad 3, bias) ->
LayerNorm -> Linear(d, 4d) -> GELU -> Linear(4d, d) -> residual.  Head: global
average pool -> LayerNorm -> Linear.

The depthwise conv runs in the ``dw::`` kernels (``ops/csrc/dwconv.hip``); the
stem and the downsamplers use the dense conv routes; channel-last LayerNorm is
the ViT's kernel on the (N*H*W, C) view, so no layout change happens anywhere.

``drop_path``: stochastic depth at rate ``drop_path * i / (blocks - 1)`` for
block ``i`` over ALL blocks, as in ``vit.py``; in training with a nonzero rate
the residual is one ``dropout_add`` kernel, otherwise a plain add.

Not covered: layer scale (timm's ``ls_init_value=None``; it is a
reparametrisation of the second Linear).
"""

from __future__ import annotations

from torch import nn

from ..ops import GELU, Conv2dNHWC, GlobalAvgPoolNHWC, LayerNorm, Linear
from ..ops.functional import dropout_add, mlp_gelu


class Block(nn.Module):
    def __init__(self, dim, drop_path=0.0):
        super().__init__()
        self.p_path = float(drop_path)
        self.dwconv = Conv2dNHWC(dim, dim, 7, padding=3, bias=True, groups=dim)
        self.norm = LayerNorm(dim)
        self.pwconv1 = Linear(dim, 4 * dim)
        self.act = GELU()
        self.pwconv2 = Linear(4 * dim, dim)

    def forward(self, x):
        # one mlp_gelu call on the two Linears' parameters; the plain add
        # goes into it (pwconv2's epilogue where the width is eligible)
        path = self.training and self.p_path > 0
        h = mlp_gelu(self.norm(self.dwconv(x)), self.pwconv1.weight,
                     self.pwconv1.bias, self.pwconv2.weight,
                     self.pwconv2.bias, None if path else x)
        return dropout_add(h, x, 0.0, self.p_path, True) if path else h


class ConvNeXt(nn.Module):
    def __init__(self, depths=(3, 3, 9, 3), dims=(96, 192, 384, 768),
                 num_classes=1000, drop_path=0.0, in_ch=3):
        super().__init__()
        assert len(depths) == len(dims)
        self.downsample = nn.ModuleList()
        self.downsample.append(nn.Sequential(
            Conv2dNHWC(in_ch, dims[0], 4, stride=4, bias=True),
            LayerNorm(dims[0]),
        ))
        for i in range(1, len(dims)):
            self.downsample.append(nn.Sequential(
                LayerNorm(dims[i - 1]),
                Conv2dNHWC(dims[i - 1], dims[i], 2, stride=2, bias=True),
            ))
        total, k = sum(depths), 0
        self.stages = nn.ModuleList()
        for depth, dim in zip(depths, dims):
            self.stages.append(nn.Sequential(*[
                Block(dim, drop_path * (k + j) / max(total - 1, 1))
                for j in range(depth)
            ]))
            k += depth
        self.pool = GlobalAvgPoolNHWC()
        self.norm = LayerNorm(dims[-1])
        self.head = Linear(dims[-1], num_classes)

    def no_weight_decay(self):
        """Biases and norm parameters are excluded by ndim <= 1 already."""
        return set()

    def forward(self, x):
        if x.dim() == 4 and x.shape[1] == 3 and x.shape[-1] != 3:
            x = x.permute(0, 2, 3, 1).contiguous()
        for down, stage in zip(self.downsample, self.stages):
            x = stage(down(x))
        return self.head(self.norm(self.pool(x)))


def convnext_tiny(num_classes=1000, drop_path=0.0):
    return ConvNeXt((3, 3, 9, 3), (96, 192, 384, 768), num_classes, drop_path)
