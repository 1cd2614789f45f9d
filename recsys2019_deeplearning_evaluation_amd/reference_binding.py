"""The device recommenders as subclasses of the REFERENCE's own base classes (last row).

The recommenders of this package are compositions `(logic mixin, device-scoring mixin, recommender base[, early stopping])`.
By default the last two are this package's re-provided copies of the reference's plugin surface (recommender_base.py), so
the package works where the reference tree is not importable.  Inside the reference tree a maintainer wants the REAL bases
-- `Base.BaseRecommender`, `Base.BaseMatrixFactorizationRecommender`, `Base.BaseSimilarityMatrixRecommender`,
`Base.Incremental_Training_Early_Stopping` -- so that `DataIO` persistence, `SearchBayesianSkopt`, `EvaluatorHoldout` and
`isinstance` checks see their own classes.  `bind()` builds exactly those subclasses:

    from Base.BaseMatrixFactorizationRecommender import BaseMatrixFactorizationRecommender
    from Base.BaseSimilarityMatrixRecommender import BaseItemSimilarityMatrixRecommender, BaseUserSimilarityMatrixRecommender
    from Base.Incremental_Training_Early_Stopping import Incremental_Training_Early_Stopping
    from recsys2019_deeplearning_evaluation_amd.reference_binding import bind
    R = bind(BaseMatrixFactorizationRecommender, BaseItemSimilarityMatrixRecommender, BaseUserSimilarityMatrixRecommender,
             Incremental_Training_Early_Stopping)
    rec = R.MatrixFactorization_BPR_MI355X(URM_train); rec.fit(epochs=300, num_factors=128, ...)

`bind(..., BaseItemCBFRecommender=..., BaseUserCBFRecommender=...)` (`Base.BaseCBFRecommender`) adds the content-based and hybrid KNN
recommenders and ItemKNNCustomSimilarityRecommender to the namespace.

`bind(..., BaseRecommender=...)` (`Base.BaseRecommender`) adds TopPop, GlobalEffects and Random.

`device_scoring=False` leaves `recommend()` to the reference's own host implementation (Base/BaseRecommender.py:131);
`EASE_R_MI355X_Recommender(..., dense_scoring="device")` then raises ValueError: the dense scorer lives in the scoring mixin.
"""
from types import SimpleNamespace

from .ease_r import _EASELogic
from .graph_based import _P3alphaLogic, _RP3betaLogic
from .ials import _IALSLogic
from .knn import _ItemKNNLogic, _UserKNNLogic
from .knn_cbf import (_ItemKNNCBFLogic, _ItemKNNCFCBFHybridLogic, _ItemKNNCustomSimilarityLogic, _UserKNNCBFLogic,
                      _UserKNNCFCBFHybridLogic)
from .matrix_factorization import _AsySVDLogic, _BPRLogic, _FunkSVDLogic
from .nmf import _NMFLogic
from .non_personalized import _GlobalEffectsLogic, _RandomLogic, _TopPopLogic
from .pure_svd import _PureSVDItemLogic, _PureSVDLogic
from .scoring import (GpuItemScoreMixin, GpuScoringMixin, GpuSimilarityScoringMixin, HandOffScoringMixin,
                      HandOffSimilarityScoringMixin)
from .slim_bpr import _SLIMLogic
from .slim_elasticnet import _SLIMElasticNetLogic


def bind(BaseMatrixFactorizationRecommender, BaseItemSimilarityMatrixRecommender, BaseUserSimilarityMatrixRecommender,
         Incremental_Training_Early_Stopping, device_scoring=True, BaseItemCBFRecommender=None, BaseUserCBFRecommender=None,
         BaseRecommender=None):
    """Returns a namespace with every recommender of this package rebuilt on the given (reference) base classes.  The content-based
    and hybrid KNN recommenders need `Base.BaseCBFRecommender`'s two classes as well: they are rebuilt when BaseItemCBFRecommender and
    BaseUserCBFRecommender are given (ItemKNNCustomSimilarityRecommender with the item pair).  The non-personalized recommenders
    (TopPop, GlobalEffects, Random) derive from `Base.BaseRecommender` itself: they are rebuilt when BaseRecommender is given."""
    mf_score = (GpuScoringMixin,) if device_scoring else ()
    sim_score = (GpuSimilarityScoringMixin,) if device_scoring else ()
    # (the recommenders that train with validations: the scoring mixin that also serves validation_hand_off = "device")
    mf = ((HandOffScoringMixin,) if device_scoring else ()) + (BaseMatrixFactorizationRecommender, Incremental_Training_Early_Stopping)
    slim_score = (HandOffSimilarityScoringMixin,) if device_scoring else ()
    table = {
        "MatrixFactorization_BPR_MI355X": (_BPRLogic,) + mf,
        "MatrixFactorization_FunkSVD_MI355X": (_FunkSVDLogic,) + mf,
        "MatrixFactorization_AsySVD_MI355X": (_AsySVDLogic,) + mf,
        "IALSRecommender": (_IALSLogic,) + mf,
        "SLIM_BPR_MI355X": (_SLIMLogic,) + slim_score + (BaseItemSimilarityMatrixRecommender, Incremental_Training_Early_Stopping),
        "SLIMElasticNetRecommender": (_SLIMElasticNetLogic,) + sim_score + (BaseItemSimilarityMatrixRecommender,),
        "PureSVDRecommender": (_PureSVDLogic,) + mf_score + (BaseMatrixFactorizationRecommender,),
        "PureSVDItemRecommender": (_PureSVDItemLogic,) + sim_score + (BaseItemSimilarityMatrixRecommender,),
        "EASE_R_MI355X_Recommender": (_EASELogic,) + sim_score + (BaseItemSimilarityMatrixRecommender,),
        "NMFRecommender": (_NMFLogic,) + mf_score + (BaseMatrixFactorizationRecommender,),
        "ItemKNNCFRecommender": (_ItemKNNLogic,) + sim_score + (BaseItemSimilarityMatrixRecommender,),
        "UserKNNCFRecommender": (_UserKNNLogic,) + sim_score + (BaseUserSimilarityMatrixRecommender,),
        "P3alphaRecommender": (_P3alphaLogic,) + sim_score + (BaseItemSimilarityMatrixRecommender,),
        "RP3betaRecommender": (_RP3betaLogic,) + sim_score + (BaseItemSimilarityMatrixRecommender,),
    }
    if BaseItemCBFRecommender is not None:
        item_cbf = sim_score + (BaseItemCBFRecommender, BaseItemSimilarityMatrixRecommender)
        table["ItemKNNCBFRecommender"] = (_ItemKNNCBFLogic,) + item_cbf
        table["ItemKNN_CFCBF_Hybrid_Recommender"] = (_ItemKNNCFCBFHybridLogic,) + item_cbf
        table["ItemKNNCustomSimilarityRecommender"] = (_ItemKNNCustomSimilarityLogic,) + sim_score + (BaseItemSimilarityMatrixRecommender,)
    if BaseUserCBFRecommender is not None:
        user_cbf = sim_score + (BaseUserCBFRecommender, BaseUserSimilarityMatrixRecommender)
        table["UserKNNCBFRecommender"] = (_UserKNNCBFLogic,) + user_cbf
        table["UserKNN_CFCBF_Hybrid_Recommender"] = (_UserKNNCFCBFHybridLogic,) + user_cbf
    if BaseRecommender is not None:
        item_score = (GpuItemScoreMixin,) if device_scoring else ()
        table["TopPop"] = (_TopPopLogic,) + item_score + (BaseRecommender,)
        table["GlobalEffects"] = (_GlobalEffectsLogic,) + item_score + (BaseRecommender,)
        table["Random"] = (_RandomLogic, BaseRecommender)                  # (scored on the host: see _RandomLogic)
    return SimpleNamespace(**{name: type(name, bases, {"__doc__": bases[0].__doc__}) for name, bases in table.items()})
