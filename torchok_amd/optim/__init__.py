from . import clip, optimizers, schedulers  # noqa: F401
from .clip import clip_grad_norm_, clip_grad_value_  # noqa: F401
