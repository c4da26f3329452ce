from .foo import FooModel
from .resnet import ResNet, resnet18, resnet50
from .convnext import ConvNeXt, convnext_tiny
from .swin import SwinTransformer, swin_tiny
from .vit import ViT, vit_b16


def is_vit(name: str) -> bool:
    return name.lower() in ("vit-b16", "vit_b16", "vitb16")


def is_convnext(name: str) -> bool:
    return name.lower() in ("convnext-t", "convnext_t", "convnext_tiny")


def is_swin(name: str) -> bool:
    return name.lower() in ("swin-t", "swin_t", "swin_tiny")


def build_model(name: str, num_classes: int | None = None,
                dropout: float = 0.0, drop_path: float = 0.0,
                attn_dropout: float = 0.0):
    """Factory used by the CLI / bench: name -> model instance.

    ``dropout`` / ``drop_path`` / ``attn_dropout`` are the ViT's regularisers
    and ``drop_path`` is also ConvNeXt's and Swin's; a nonzero rate with any
    other model is an error."""
    name = name.lower()
    if (dropout or attn_dropout) and not is_vit(name):
        raise ValueError(
            "dropout / attn_dropout are only wired into the ViT, "
            f"not {name!r}"
        )
    if drop_path and not (is_vit(name) or is_convnext(name) or is_swin(name)):
        raise ValueError(
            "drop_path is only wired into the ViT, ConvNeXt and Swin, "
            f"not {name!r}"
        )
    if name in ("foo", "foomodel", "mlp"):
        return FooModel()
    if name in ("resnet18", "resnet18-cifar"):
        return resnet18(num_classes or 10, stem="cifar")
    if name == "resnet18-imagenet":
        return resnet18(num_classes or 1000, stem="imagenet")
    if name == "resnet50":
        return resnet50(num_classes or 1000, stem="imagenet")
    if is_vit(name):
        return vit_b16(num_classes or 1000, dropout=dropout,
                       drop_path=drop_path, attn_dropout=attn_dropout)
    if is_convnext(name):
        return convnext_tiny(num_classes or 1000, drop_path=drop_path)
    if is_swin(name):
        return swin_tiny(num_classes or 1000, drop_path=drop_path)
    raise ValueError(f"unknown model {name!r}")


__all__ = [
    "FooModel",
    "ResNet",
    "resnet18",
    "resnet50",
    "ViT",
    "vit_b16",
    "ConvNeXt",
    "convnext_tiny",
    "SwinTransformer",
    "swin_tiny",
    "build_model",
]
