from . import davit, efficientnet, hrnet, resnet, swin  # noqa: F401
