from . import beit, davit, efficientnet, hrnet, mobilenetv3, resnet, swin, vit  # noqa: F401
