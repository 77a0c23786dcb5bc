from . import davit, efficientnet, hrnet, resnet, swin, vit  # noqa: F401
