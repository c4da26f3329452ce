from .foo import FooModel
from .resnet import ResNet, resnet18, resnet50
from .vit import ViT, vit_b16


def is_vit(name: str) -> bool:
    return name.lower() in ("vit-b16", "vit_b16", "vitb16")


def build_model(name: str, num_classes: int | None = None,
                dropout: float = 0.0, drop_path: float = 0.0):
    """Factory used by the CLI / bench: name -> model instance.

    ``dropout`` / ``drop_path`` are the ViT's regularisers; a nonzero rate
    with any other model is an error."""
    name = name.lower()
    if (dropout or drop_path) and not is_vit(name):
        raise ValueError(
            f"dropout / drop_path are only wired into the ViT, not {name!r}"
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
                       drop_path=drop_path)
    raise ValueError(f"unknown model {name!r}")


__all__ = [
    "FooModel",
    "ResNet",
    "resnet18",
    "resnet50",
    "ViT",
    "vit_b16",
    "build_model",
]
