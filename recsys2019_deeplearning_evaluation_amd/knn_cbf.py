"""Content-based and CF+CBF hybrid KNN recommenders whose similarity build runs on MI355X.

Mirrors KNN/ItemKNNCBFRecommender.py:18 (fit :30-51), KNN/UserKNNCBFRecommender.py:18 (fit :29-50),
KNN/ItemKNN_CFCBF_Hybrid_Recommender.py:15 (fit :20-25), KNN/UserKNN_CFCBF_Hybrid_Recommender.py:16 (fit :21-26) and
KNN/ItemKNNCustomSimilarityRecommender.py:15 (fit :20-33): same constructors, same fit() keywords, same W_sparse and post-fit
ICM_train / UCM_train attributes, same scoring through the base classes.

The dataMatrix of a content-based build is `ICM_train.T` (n_features x n_items): few, long rows of real values, empty columns for
items without features.  It is the transpose of a CSR matrix, i.e. CSC, so the reference sums the squares behind the norms in the
CSC order (include/mi355rec.h, norm_sum_order = 1); the matrix is handed on as that transpose.  BM25 / TF-IDF weight the rows of the
ICM -- the COLUMNS of the dataMatrix -- in the constructor's device pre-pass.

A hybrid stacks the weighted content matrix on the interactions: `hstack([ICM_train * ICM_weight, URM_train.T])`.  Done the
reference's way that is three SciPy passes over every stored cell plus an upload per fit, around a build of a few milliseconds; a
search changes nothing but the weight between fits.  `fit(..., resident_blocks=(...))` takes the two blocks from device memory
(`ResidentURM`s uploaded once) and scales and stacks them there (`ResidentStack`, csrc/stack.hip).
"""
import numpy as np
import scipy.sparse as sps

from . import _native as N
from .knn import _KNNCFMixin
from .recommender_base import (BaseItemCBFRecommender, BaseItemSimilarityMatrixRecommender, BaseUserCBFRecommender,
                               BaseUserSimilarityMatrixRecommender, check_matrix, similarityMatrixTopK)
from .scoring import GpuSimilarityScoringMixin
from .similarity import Compute_Similarity, Compute_Similarity_MI355X


class _KNNCBFLogic(_KNNCFMixin):
    """What the four feature-taking recommenders share.  `_CM` names the content-matrix attribute (ICM_train / UCM_train)."""
    _CM = None

    def _fit_on_content_matrix(self, topK, shrink, similarity, normalize, feature_weighting, similarity_args):
        self.topK = topK
        self.shrink = shrink
        self._check_weighting(feature_weighting)
        CM = getattr(self, self._CM)
        # okapi_BM_25(ICM) / TF_IDF(ICM) (ItemKNNCBFRecommender.py:39-45): documents = rows of the content matrix = columns of its transpose
        builder = Compute_Similarity(CM.T, shrink=shrink, topK=topK, normalize=normalize, similarity=similarity,
                                     feature_weighting=feature_weighting, weighting_documents="columns", **similarity_args)
        if feature_weighting != "none":
            setattr(self, self._CM, check_matrix(builder.compute_similarity_object.weighted_matrix().T, "csr"))
        self._finish_build(builder.compute_similarity_object)

    def _finish_build(self, sim):
        self.W_sparse = check_matrix(sim.compute_similarity(), format="csr")
        self.similarity_stats = sim.stats()
        sim.close()


class _ItemKNNCBFLogic(_KNNCBFLogic):
    """ItemKNN content-based recommender: W_sparse = top-K item-item similarity of the ICM rows."""
    RECOMMENDER_NAME = "ItemKNNCBFRecommender"
    _CM = "ICM_train"

    def __init__(self, URM_train, ICM_train, verbose=True):
        super(_ItemKNNCBFLogic, self).__init__(URM_train, ICM_train, verbose=verbose)

    def fit(self, topK=50, shrink=100, similarity="cosine", normalize=True, feature_weighting="none", **similarity_args):
        self._fit_on_content_matrix(topK, shrink, similarity, normalize, feature_weighting, similarity_args)


class _UserKNNCBFLogic(_KNNCBFLogic):
    """UserKNN content-based recommender: W_sparse = top-K user-user similarity of the UCM rows; user bases wider than the LDS
    accumulator (32 256 cells) are handled by the kernel's accumulator tiling."""
    RECOMMENDER_NAME = "UserKNNCBFRecommender"
    _SCORER_USER_BASED = True
    _CM = "UCM_train"

    def __init__(self, URM_train, UCM_train, verbose=True):
        super(_UserKNNCBFLogic, self).__init__(URM_train, UCM_train, verbose=verbose)

    def fit(self, topK=50, shrink=100, similarity="cosine", normalize=True, feature_weighting="none", **similarity_args):
        self._fit_on_content_matrix(topK, shrink, similarity, normalize, feature_weighting, similarity_args)


class _HybridLogic:
    """The CF+CBF stacking of the two hybrids.  Subclasses say which matrix of interactions goes next to the content matrix
    (`_interactions()`: URM_train.T for items, URM_train for users)."""

    def _interactions(self):
        raise NotImplementedError()

    def _host_stack(self, weight):
        """hstack([CM * weight, interactions]) as the reference makes it (ItemKNN_CFCBF_Hybrid_Recommender.py:22-23): CSR float32."""
        return sps.hstack([getattr(self, self._CM) * weight, self._interactions()], format="csr")

    def _hybrid_fit(self, weight, resident_blocks, fit_args):
        if resident_blocks is None or fit_args.get("similarity") == "euclidean":       # (the Euclidean front-end uploads its own, squared, copy)
            setattr(self, self._CM, self._host_stack(weight))
            self._resident_fit = None
            return self._fit_on_content_matrix(**self._fit_keywords(**fit_args))
        self._fit_on_resident_blocks(weight, resident_blocks, **self._fit_keywords(**fit_args))

    @staticmethod
    def _fit_keywords(topK=50, shrink=100, similarity="cosine", normalize=True, feature_weighting="none", **similarity_args):
        return dict(topK=topK, shrink=shrink, similarity=similarity, normalize=normalize, feature_weighting=feature_weighting,
                    similarity_args=similarity_args)

    def _fit_on_resident_blocks(self, weight, resident_blocks, topK, shrink, similarity, normalize, feature_weighting, similarity_args):
        """The dataMatrix -- content rows times `weight` on top of the interaction rows -- is scaled and stacked in device memory from
        blocks that are already there; nothing proportional to the stored cells happens on the host."""
        self.topK = topK
        self.shrink = shrink
        self._check_weighting(feature_weighting)
        content, interactions = resident_blocks
        if not content.matches_transposed(getattr(self, self._CM)):
            raise ValueError("{}: resident_blocks[0] does not hold {}.T (shape, nnz or contents differ; make it from the CSC "
                             "transpose: ResidentURM({}.T))".format(self.RECOMMENDER_NAME, self._CM, self._CM))
        if not self._interactions_match(interactions):
            raise ValueError("{}: resident_blocks[1] does not hold the interactions of URM_train (shape, nnz or contents differ)".format(
                self.RECOMMENDER_NAME))
        similarity_args = dict(similarity_args)
        use_implementation = similarity_args.pop("use_implementation", "density")
        stack = N.ResidentStack([content, interactions], [weight, 1.0])
        try:
            Compute_Similarity.check_request(stack.shape, stack.nnz, similarity, use_implementation)
            try:
                # the reference is handed hstack(...).T, a CSC matrix: its norms are summed in the CSC order
                sim = Compute_Similarity_MI355X.from_resident(stack, 1, shrink=shrink, topK=topK, normalize=normalize, similarity=similarity,
                                                              feature_weighting=feature_weighting, weighting_documents="columns",
                                                              **similarity_args)
            except ValueError as exc:
                if "non finite" in str(exc):
                    raise AssertionError("Compute_Similarity: Data matrix contains {} non finite values".format(
                        stack.count_non_finite())) from None
                raise
            self._resident_fit = (weight, feature_weighting, sim.weighted_matrix() if feature_weighting != "none" else None)
            self._finish_build(sim)
        finally:
            stack.close()

    def stacked_matrix(self):
        """What the reference keeps as ICM_train / UCM_train after this fit: hstack([CM * weight, interactions]), re-weighted where the
        fit asked for it.  After a fit with `resident_blocks` the attribute itself keeps the constructor's matrix and this is made
        on demand; after a host-stacked fit it IS the attribute."""
        if getattr(self, "_resident_fit", None) is None:
            return getattr(self, self._CM)
        weight, feature_weighting, weighted = self._resident_fit
        return self._host_stack(weight) if weighted is None else check_matrix(weighted.T, "csr")


class _ItemKNNCFCBFHybridLogic(_HybridLogic, _ItemKNNCBFLogic):
    """ItemKNN on hstack([ICM_train * ICM_weight, URM_train.T]): content and collaborative evidence in one similarity."""
    RECOMMENDER_NAME = "ItemKNN_CFCBF_HybridRecommender"

    def fit(self, ICM_weight=1.0, resident_blocks=None, **fit_args):
        """resident_blocks (not an argument of the reference): `(ResidentURM(ICM_train.T), ResidentURM(URM_train))`, uploaded once for a
        whole search -- the stack is then made on the device (both are verified against this recommender's matrices).  ICM_train
        keeps the constructor's matrix in that mode; `stacked_matrix()` gives the reference's post-fit value.  With
        similarity="euclidean" the blocks are ignored (neither used nor verified) and the fit stacks on the host: that front-end squares
        the values on the host and uploads its own copy, as it ignores `resident_urm` in ItemKNNCFRecommender."""
        self._hybrid_fit(ICM_weight, resident_blocks, fit_args)

    def _interactions(self):
        return self.URM_train.T

    def _interactions_match(self, block):
        return block.matches(self.URM_train)

    def _get_cold_item_mask(self):
        return np.logical_and(self._cold_item_CBF_mask, self._cold_item_mask)


class _UserKNNCFCBFHybridLogic(_HybridLogic, _UserKNNCBFLogic):
    """UserKNN on hstack([UCM_train * UCM_weight, URM_train])."""
    RECOMMENDER_NAME = "UserKNN_CFCBF_Hybrid_Recommender"

    def fit(self, UCM_weight=1.0, resident_blocks=None, **fit_args):
        """resident_blocks (not an argument of the reference): `(ResidentURM(UCM_train.T), ResidentURM(URM_train.T))`; see
        ItemKNN_CFCBF_Hybrid_Recommender.fit."""
        self._hybrid_fit(UCM_weight, resident_blocks, fit_args)

    def _interactions(self):
        return self.URM_train

    def _interactions_match(self, block):
        return block.matches_transposed(self.URM_train)

    def _get_cold_user_mask(self):
        return np.logical_and(self._cold_user_CBF_mask, self._cold_user_mask)


class _ItemKNNCustomSimilarityLogic:
    """ItemKNN scoring over an item-item similarity the caller provides."""
    RECOMMENDER_NAME = "ItemKNNCustomSimilarityRecommender"

    def fit(self, W_sparse, selectTopK=False, topK=100):
        """W_sparse: (n_items, n_items), column = source item as everywhere in this package; selectTopK keeps the topK largest
        non-zero cells of every column."""
        n = self.URM_train.shape[1]
        if W_sparse.shape[0] != W_sparse.shape[1]:
            raise AssertionError("{}: the similarity is not square, its shape is {}".format(self.RECOMMENDER_NAME, W_sparse.shape))
        if W_sparse.shape != (n, n):
            raise AssertionError("{}: the similarity is not consistent with URM_train: {} for {} items".format(
                self.RECOMMENDER_NAME, W_sparse.shape, n))
        kept = similarityMatrixTopK(W_sparse, k=topK) if selectTopK else W_sparse
        self.W_sparse = check_matrix(kept, format="csr")


class ItemKNNCBFRecommender(_ItemKNNCBFLogic, GpuSimilarityScoringMixin, BaseItemCBFRecommender, BaseItemSimilarityMatrixRecommender):
    pass


class UserKNNCBFRecommender(_UserKNNCBFLogic, GpuSimilarityScoringMixin, BaseUserCBFRecommender, BaseUserSimilarityMatrixRecommender):
    pass


class ItemKNN_CFCBF_Hybrid_Recommender(_ItemKNNCFCBFHybridLogic, GpuSimilarityScoringMixin, BaseItemCBFRecommender,
                                       BaseItemSimilarityMatrixRecommender):
    pass


class UserKNN_CFCBF_Hybrid_Recommender(_UserKNNCFCBFHybridLogic, GpuSimilarityScoringMixin, BaseUserCBFRecommender,
                                       BaseUserSimilarityMatrixRecommender):
    pass


class ItemKNNCustomSimilarityRecommender(_ItemKNNCustomSimilarityLogic, GpuSimilarityScoringMixin, BaseItemSimilarityMatrixRecommender):
    pass
