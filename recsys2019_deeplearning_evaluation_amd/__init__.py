"""MI355X-native (gfx950) training kernels for the baseline recommenders of
MaurizioFD/RecSys2019_DeepLearning_Evaluation, behind the reference's own recommender surface.

Hot path only: Compute_Similarity (ItemKNN build), BPR-MF / FunkSVD SGD epochs, SLIM-BPR epoch,
IALS solve step, SLIM ElasticNet coordinate descent, PureSVD's randomized SVD, NMF's coordinate-descent and multiplicative-update solvers.  Python host code + ctypes C-ABI (include/mi355rec.h) + hand-written HIP kernels (csrc/).
Nothing here imports torch; torch.distributed is only used by `sharding` for the multi-GPU gather.
"""
from ._native import ResidentURM, ResidentStack  # noqa: F401
from .similarity import Compute_Similarity, Compute_Similarity_MI355X, Compute_Similarity_Euclidean_MI355X  # noqa: F401
from .knn import ItemKNNCFRecommender, UserKNNCFRecommender  # noqa: F401
from .knn_cbf import (ItemKNNCBFRecommender, UserKNNCBFRecommender, ItemKNN_CFCBF_Hybrid_Recommender,  # noqa: F401
                      UserKNN_CFCBF_Hybrid_Recommender, ItemKNNCustomSimilarityRecommender)
from .matrix_factorization import (MatrixFactorization_MI355X_Epoch, MatrixFactorization_BPR_MI355X,  # noqa: F401
                                   MatrixFactorization_FunkSVD_MI355X, MatrixFactorization_AsySVD_MI355X,
                                   MatrixFactorization_MI355X_Group, asysvd_user_factors)

from .slim_bpr import SLIM_BPR_MI355X_Epoch, SLIM_BPR_MI355X  # noqa: F401,E402
from .scoring import (MI355XScorer, MI355XSparseScorer, MI355XDenseScorer, MI355XItemScorer, GpuScoringMixin, GpuSimilarityScoringMixin,  # noqa: F401,E402
                      GpuItemScoreMixin)
from .graph_based import P3alphaRecommender, RP3betaRecommender  # noqa: F401,E402
from .ease_r import EASE_R_Recommender, EASE_R_MI355X_Recommender, MI355XEase  # noqa: F401,E402
from .ials import IALS_MI355X_Epoch, IALSRecommender  # noqa: F401,E402
from .slim_elasticnet import SLIMElasticNetRecommender  # noqa: F401,E402
from .evaluation import EvaluatorHoldout_MI355X, EvaluatorNegativeItemSample_MI355X  # noqa: F401,E402
from .pure_svd import PureSVDRecommender, PureSVDItemRecommender  # noqa: F401,E402
from .nmf import NMFRecommender  # noqa: F401,E402
from .non_personalized import TopPop, GlobalEffects, Random  # noqa: F401,E402

__all__ = ["MI355XDenseScorer", "TopPop", "GlobalEffects", "Random", "MI355XItemScorer", "GpuItemScoreMixin", "ResidentURM", "ResidentStack", "ItemKNNCBFRecommender", "UserKNNCBFRecommender", "ItemKNN_CFCBF_Hybrid_Recommender", "UserKNN_CFCBF_Hybrid_Recommender", "ItemKNNCustomSimilarityRecommender", "PureSVDRecommender", "PureSVDItemRecommender", "NMFRecommender", "EvaluatorHoldout_MI355X", "EvaluatorNegativeItemSample_MI355X", "EASE_R_Recommender", "EASE_R_MI355X_Recommender", "MI355XEase", "SLIMElasticNetRecommender", "P3alphaRecommender", "RP3betaRecommender", "MI355XScorer", "MI355XSparseScorer", "GpuScoringMixin", "GpuSimilarityScoringMixin", "SLIM_BPR_MI355X_Epoch", "SLIM_BPR_MI355X", "IALS_MI355X_Epoch", "IALSRecommender", "Compute_Similarity", "Compute_Similarity_MI355X", "Compute_Similarity_Euclidean_MI355X", "ItemKNNCFRecommender", "UserKNNCFRecommender",
           "MatrixFactorization_MI355X_Epoch", "MatrixFactorization_MI355X_Group", "MatrixFactorization_BPR_MI355X", "MatrixFactorization_FunkSVD_MI355X", "MatrixFactorization_AsySVD_MI355X", "asysvd_user_factors"]
