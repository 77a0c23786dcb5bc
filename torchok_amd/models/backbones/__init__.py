from . import beit, davit, efficientnet, gcvit, hrnet, mobilenetv3, resnet, swin, vit  # noqa: F401
