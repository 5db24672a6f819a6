"""Loss functions and retrieval metrics of the reference's ``multimodal`` workflow on the gfx950 kernels."""
from .contrastive_loss import HyperbolicInfoNCE, hyperbolic_contrastive_loss, hyperbolic_triplet_loss  # noqa: F401
from .retrieval import compute_recall_at_k, hyperbolic_knn, retrieval_ranks  # noqa: F401
