"""Loss functions of the reference's ``multimodal`` package on the gfx950 kernels."""
from .contrastive_loss import HyperbolicInfoNCE, hyperbolic_contrastive_loss, hyperbolic_triplet_loss  # noqa: F401
