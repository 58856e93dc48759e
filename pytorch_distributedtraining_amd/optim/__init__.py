"""Optimizer-side components: fused AdamW / SGD / LAMB, fused grad clipping, loss scaling."""
from ._fused import FusedOptimizer
from .clip import clip_grad_norm_, grad_norm_sq
from .fused_adamw import FusedAdamW
from .fused_lamb import FusedLAMB
from .fused_sgd import FusedSGD
from .grad_scaler import GradScaler

__all__ = ["FusedOptimizer", "FusedAdamW", "FusedLAMB", "FusedSGD", "clip_grad_norm_", "grad_norm_sq", "GradScaler"]
