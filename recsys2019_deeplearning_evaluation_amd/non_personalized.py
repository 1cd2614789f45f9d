"""The reference's non-personalized recommenders -- the baselines every table of its study is read against -- with their fit and
their ranking on MI355X.

Mirrors Base/NonPersonalizedRecommender.py: TopPop (:14, fit :23-27), GlobalEffects (:62, fit :71-116) and Random (:151): same
RECOMMENDER_NAME, fit() keywords, attributes and save_model dictionaries.  All three give every user the same kind of score row, so
they cost nothing to train and everything to evaluate: the reference repeats one vector of n_items scores for every user of a block
and partitions and sorts each copy.  Here `GpuItemScoreMixin` sorts the vector once and hands each user the head of that order
without the user's seen items (csrc/itemscore.hip).  The fits read URM_train as the CSR matrix it is -- column counts and column
sums without a CSC copy (csrc/nonpers.hip).  `_compute_item_score` stays the host statement of the reference's, so either path can
be checked against the other.
"""
import ctypes as C

import numpy as np

from . import _native as N
from .recommender_base import BaseRecommender
from .scoring import GpuItemScoreMixin


def _check_resident(recommender, resident_urm):
    if resident_urm is not None and not resident_urm.matches(recommender.URM_train):
        raise ValueError("{}: resident_urm does not hold this recommender's URM_train".format(recommender.RECOMMENDER_NAME))
    return resident_urm


def _csr_arrays(URM):
    return N.as_i32(URM.indptr), N.as_i32(URM.indices), N.as_f32(URM.data)


def urm_item_counts(URM_train, resident_urm=None):
    """Stored cells per column of a CSR matrix, int32 (np.ediff1d(URM.tocsc().indptr)), counted on the device."""
    n_users, n_items = URM_train.shape
    counts = np.zeros(n_items, np.int32)
    lib = N.load()
    if resident_urm is not None:
        N.check(lib.mi355rec_urm_item_counts_resident(n_users, n_items, resident_urm.nnz, resident_urm.indptr.ptr, resident_urm.indices.ptr,
                                                      N.ptr(counts)))
    else:
        indptr, indices, _ = _csr_arrays(URM_train)
        N.check(lib.mi355rec_urm_item_counts(n_users, n_items, N.ptr(indptr), N.ptr(indices), N.ptr(counts)))
    return counts


def urm_global_effects(URM_train, lambda_user, lambda_item, resident_urm=None):
    """(mu float32, item_bias float64[n_items], user_bias float64[n_users]) of GlobalEffects.fit, computed on the device."""
    n_users, n_items = URM_train.shape
    mu = C.c_float(0.0)
    item_bias, user_bias = np.zeros(n_items, np.float64), np.zeros(n_users, np.float64)
    lib = N.load()
    if resident_urm is not None:
        N.check(lib.mi355rec_urm_global_effects_resident(n_users, n_items, resident_urm.nnz, resident_urm.indptr.ptr, resident_urm.indices.ptr,
                                                         resident_urm.data.ptr, float(lambda_user), float(lambda_item), C.byref(mu),
                                                         N.ptr(item_bias), N.ptr(user_bias)))
    else:
        indptr, indices, data = _csr_arrays(URM_train)
        N.check(lib.mi355rec_urm_global_effects(n_users, n_items, N.ptr(indptr), N.ptr(indices), N.ptr(data), float(lambda_user),
                                                float(lambda_item), C.byref(mu), N.ptr(item_bias), N.ptr(user_bias)))
    return np.float32(mu.value), item_bias, user_bias


def _repeat_for_users(vector, n_items, user_id_array, items_to_compute, dtype):
    """The score block of a model with one score per item: the vector (or, with items_to_compute, a float32 row of -inf that holds
    the vector at those items only) as `dtype`, one copy per user."""
    if items_to_compute is None:
        row = np.array(vector, copy=True)
    else:
        row = np.full(n_items, -np.inf, dtype=np.float32)
        row[items_to_compute] = vector[items_to_compute]
    return np.repeat(np.array(row, dtype=dtype).reshape(1, -1), len(user_id_array), axis=0)


def _save(recommender, folder_path, file_name, data):
    """Through this package's BaseRecommender, or -- bound to the reference's -- through the reference's DataIO."""
    if hasattr(recommender, "_save_dict"):
        recommender._save_dict(folder_path, file_name, data)
        return
    from Base.DataIO import DataIO
    name = recommender.RECOMMENDER_NAME if file_name is None else file_name
    recommender._print("Saving model in file '{}'".format(folder_path + name))
    DataIO(folder_path=folder_path).save_data(file_name=name, data_dict_to_save=data)
    recommender._print("Saving complete")


class _TopPopLogic:
    """Top Popular recommender: every user is offered the items with the most interactions.  `item_pop` (int32) holds the stored
    cells of every column of URM_train."""
    RECOMMENDER_NAME = "TopPopRecommender"

    def __init__(self, URM_train, verbose=True):
        super(_TopPopLogic, self).__init__(URM_train, verbose=verbose)

    def fit(self, resident_urm=None):
        """resident_urm (not an argument of the reference): a `ResidentURM` of this URM_train -- the counts are taken from the device
        copy, which also serves as the scorer's seen CSR."""
        self._resident_urm = _check_resident(self, resident_urm)
        self.item_pop = urm_item_counts(self.URM_train, self._resident_urm)
        self.n_items = self.URM_train.shape[1]

    def _item_score_vector(self):
        return self.item_pop

    def _compute_item_score(self, user_id_array, items_to_compute=None):
        return _repeat_for_users(self.item_pop, self.n_items, user_id_array, items_to_compute, np.float32)

    def save_model(self, folder_path, file_name=None):
        _save(self, folder_path, file_name, {"item_pop": self.item_pop})


class _GlobalEffectsLogic:
    """Global effects: mu, the global mean rating; item_bias, the damped mean of every item's ratings around mu; user_bias, the damped
    mean of what is left of every user's ratings.  Items are ranked by item_bias alone (mu and user_bias do not change a user's order).

    Stated deviations from the reference.  (1) The device ranks float32(item_bias) where the reference's recommend() without
    items_to_compute ranks the float64 vector: items whose biases differ by less than a float32 ulp become ties and go to the lower
    item id.  (With items_to_compute the reference ranks float32 values as well.)  (2) The reference sums the centred ratings in
    float32 (scipy's sum of a float32 matrix); here every sum is float64 in a fixed order, with the reference's element-wise float32
    roundings.  (3) user_bias is a 1-D array; the reference's is a 1 x n_users np.matrix."""
    RECOMMENDER_NAME = "GlobalEffectsRecommender"

    def __init__(self, URM_train, verbose=True):
        super(_GlobalEffectsLogic, self).__init__(URM_train, verbose=verbose)

    def fit(self, lambda_user=10, lambda_item=25, resident_urm=None):
        """resident_urm (not an argument of the reference): as for TopPop."""
        self.lambda_user = lambda_user
        self.lambda_item = lambda_item
        self.n_items = self.URM_train.shape[1]
        self._resident_urm = _check_resident(self, resident_urm)
        self.mu, self.item_bias, self.user_bias = urm_global_effects(self.URM_train, lambda_user, lambda_item, self._resident_urm)

    def _item_score_vector(self):
        return self.item_bias

    def _compute_item_score(self, user_id_array, items_to_compute=None):
        return _repeat_for_users(self.item_bias, self.n_items, user_id_array, items_to_compute, np.float64)

    def save_model(self, folder_path, file_name=None):
        _save(self, folder_path, file_name, {"item_bias": self.item_bias})


class _RandomLogic:
    """Random recommender.  It stays on the host on purpose: its scores ARE the reference's `np.random` stream, drawn per call as
    float64 -- fit() seeds the global generator, every _compute_item_score draws one block from it -- and a device ranking of a
    float32 copy would reorder near-equal draws.  It uses BaseRecommender.recommend as it is and needs no device."""
    RECOMMENDER_NAME = "RandomRecommender"

    def __init__(self, URM_train, verbose=True):
        super(_RandomLogic, self).__init__(URM_train, verbose=verbose)

    def fit(self, random_seed=42):
        np.random.seed(random_seed)
        self.n_items = self.URM_train.shape[1]

    def _compute_item_score(self, user_id_array, items_to_compute=None):
        n = len(user_id_array)
        if items_to_compute is None:
            return np.random.rand(n, self.n_items)
        item_scores = np.full((n, self.n_items), -np.inf, dtype=np.float32)
        item_scores[:, items_to_compute] = np.random.rand(n, len(items_to_compute))
        return item_scores

    def save_model(self, folder_path, file_name=None):
        _save(self, folder_path, file_name, {})


class TopPop(_TopPopLogic, GpuItemScoreMixin, BaseRecommender):
    __doc__ = _TopPopLogic.__doc__


class GlobalEffects(_GlobalEffectsLogic, GpuItemScoreMixin, BaseRecommender):
    __doc__ = _GlobalEffectsLogic.__doc__


class Random(_RandomLogic, BaseRecommender):
    __doc__ = _RandomLogic.__doc__
