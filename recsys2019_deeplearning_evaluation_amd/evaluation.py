"""Holdout evaluation on the MI355X: the reference's EvaluatorHoldout (Base/Evaluation/Evaluator.py:141-211, 382-450) with the
per-user metric loop (:294-374, Base/Evaluation/metrics.py) run by a HIP kernel over ranked lists in HBM.

`EvaluatorHoldout_MI355X` takes the reference's constructor arguments and returns the reference's `(results_dict, results_string)`,
so early stopping (`Incremental_Training_Early_Stopping._train_with_early_stopping`) and the reference's search classes take it as
their `evaluator_object` unchanged.  Two paths:
  fused  recommenders with a device scorer (GpuScoringMixin / GpuSimilarityScoringMixin / GpuItemScoreMixin): each block of users is scored,
         ranked and evaluated on the device; neither scores nor lists reach the host.
  lists  any other recommender: recommend(..., return_scores=False) on the host, the lists uploaded, the same metric kernel.
`EvaluatorNegativeItemSample_MI355X` is the reference's EvaluatorNegativeItemSample (Evaluator.py:455-539) on the same two paths: every
user ranks its own candidates only (its test items plus the sampled negatives), the metrics are the parent's.
Given the same lists, both give bitwise the same result, whatever the block size.  (The sparse scorer sums with LDS float atomics, so
its order of near-tied scores, and with it a list, can change from one call to the next.)  O(n_items) population metrics (coverage, Gini, Shannon,
Herfindahl, mean inter-list diversity) and F1 are finished here in float64 from the device's item counters.
With a `diversity_object` (the reference's Diversity_similarity, or a dense ndarray) both evaluators add DIVERSITY_SIMILARITY
(metrics.py:641-694): the matrix is uploaded once, at construction, and a second kernel behind the metric kernel gathers each list's
cells from it in float64 (csrc/eval_diversity.cuh).  Where the reference raises ZeroDivisionError -- a list of fewer than two items
at some cutoff -- so does evaluateRecommender, after the evaluation.  Deviation: the matrix's range is checked once, at construction,
on the device (ValueError), not on every evaluation.
"""
import ctypes as C
import sys
import time

import numpy as np
import scipy.sparse as sps

from . import _native as N
from .scoring import _ScoringMixin, allowed_items

# EvaluatorMetrics order (Evaluator.py:20-40), without DIVERSITY_SIMILARITY
METRICS = ["ROC_AUC", "PRECISION", "PRECISION_RECALL_MIN_DEN", "RECALL", "MAP", "MRR", "NDCG", "F1", "HIT_RATE", "ARHR", "NOVELTY",
           "AVERAGE_POPULARITY", "DIVERSITY_MEAN_INTER_LIST", "DIVERSITY_HERFINDAHL", "COVERAGE_ITEM", "COVERAGE_USER",
           "DIVERSITY_GINI", "SHANNON_ENTROPY"]
# the per-user values of the device, in MI355REC_EVAL_VALUES order; the last one (list not empty) feeds COVERAGE_USER
PER_USER = ["ROC_AUC", "PRECISION", "PRECISION_RECALL_MIN_DEN", "RECALL", "MAP", "MRR", "NDCG", "HIT_RATE", "ARHR", "NOVELTY",
            "AVERAGE_POPULARITY"]
N_VALUES = len(PER_USER) + 1
# With a diversity_object: the metric at its place in EvaluatorMetrics, after AVERAGE_POPULARITY (Evaluator.py:34-36)
DIVERSITY_SIMILARITY = "DIVERSITY_SIMILARITY"
METRICS_WITH_DIVERSITY = (METRICS[:METRICS.index("AVERAGE_POPULARITY") + 1] + [DIVERSITY_SIMILARITY]
                          + METRICS[METRICS.index("AVERAGE_POPULARITY") + 1:])
DIVERSITY_MAX_WIDTH = 1024          # csrc/eval_plan.h DIV_MAX_WIDTH


def diversity_matrix_of(diversity_object, n_items, check_values=True):
    """The item diversity matrix of a `diversity_object` as the device takes it: a C-contiguous n_items x n_items ndarray, float32 or
    float64 as passed, any other real dtype as float64.  Accepted: an object with an `item_diversity_matrix` attribute (the
    reference's Diversity_similarity, metrics.py:641-661) or a bare ndarray.  Anything else, a scipy sparse matrix and np.matrix
    raise NotImplementedError; a wrong shape, a value outside [0, 1] and a NaN raise ValueError (the assertion of metrics.py:655-656,
    which the reference makes in Diversity_similarity.__init__).  Needs no device.  check_values=False leaves the range to the caller:
    the evaluators check it on the device after the upload."""
    matrix = getattr(diversity_object, "item_diversity_matrix", diversity_object)
    if sps.issparse(matrix) or isinstance(matrix, np.matrix) or not isinstance(matrix, np.ndarray) or matrix.dtype.kind not in "fiub":
        raise NotImplementedError("DIVERSITY_SIMILARITY takes a dense numpy.ndarray of real numbers, or an object whose "
                                  "`item_diversity_matrix` is one (Diversity_similarity): got {}".format(type(matrix).__name__))
    if matrix.ndim != 2 or matrix.shape != (n_items, n_items):
        raise ValueError("item_diversity_matrix is {}, expected {}".format(matrix.shape, (n_items, n_items)))
    if matrix.dtype not in (np.float32, np.float64):
        matrix = matrix.astype(np.float64)
    matrix = np.ascontiguousarray(matrix)
    if check_values and matrix.size and not (np.all(matrix >= 0.0) and np.all(matrix <= 1.0)):      # (a NaN fails both comparisons)
        raise ValueError("item_diversity_matrix contains value greater than 1.0 or lower than 0.0")
    return matrix


def get_result_string(results_run, n_decimals=7):
    """Evaluator.py:105-121."""
    output_str = ""
    for cutoff in results_run.keys():
        output_str += "CUTOFF: {} - ".format(cutoff)
        for metric, value in results_run[cutoff].items():
            output_str += "{}: {:.{n_decimals}f}, ".format(metric, value, n_decimals=n_decimals)
        output_str += "\n"
    return output_str


def population_metrics(counter, n_evaluated_users, cutoff, ignore_items, n_users, n_ignore_users, n_covered):
    """The metrics of one cutoff that need the whole recommended-item counter (metrics.py:272-371, 400-529, 700-789), in float64, written as
    the reference writes them.  counter: times each item was recommended within the cutoff."""
    counter = np.asarray(counter, dtype=np.float64)
    keep = np.ones(len(counter), dtype=bool)
    keep[np.asarray(ignore_items, dtype=np.int64)] = False
    kept = counter[keep]                                                        # _get_recommended_items_counter (:288-297)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        # Diversity_MeanInterList.get_metric_value (:774-789): the nominal cutoff, ignored items included
        if n_evaluated_users == 0:
            out["DIVERSITY_MEAN_INTER_LIST"] = 1.0
        else:
            cooccurrences_cumulative = np.sum(counter ** 2) - n_evaluated_users * cutoff
            all_user_couples_count = n_evaluated_users ** 2 - n_evaluated_users
            diversity_cumulative = all_user_couples_count - cooccurrences_cumulative / cutoff
            out["DIVERSITY_MEAN_INTER_LIST"] = diversity_cumulative / np.float64(all_user_couples_count)
        # _compute_diversity_herfindahl (:471-478)
        out["DIVERSITY_HERFINDAHL"] = 1 - np.sum((kept / kept.sum()) ** 2) if kept.sum() != 0 else np.nan
        # Coverage_Item.get_metric_value (:320-324)
        recommended_mask = kept > 0
        out["COVERAGE_ITEM"] = recommended_mask.sum() / len(recommended_mask)
        # Coverage_User.get_metric_value (:364-365)
        out["COVERAGE_USER"] = n_covered / (n_users - n_ignore_users)
        # _compute_diversity_gini (:425-441)
        n = len(kept)
        ordered = np.sort(kept)
        index = np.arange(1, n + 1)
        out["DIVERSITY_GINI"] = 2 * np.sum((n + 1 - index) / (n + 1) * ordered / np.sum(ordered))
        # _compute_shannon_entropy (:514-529)
        nonzero = kept[kept != 0]
        probability = nonzero / nonzero.sum()
        out["SHANNON_ENTROPY"] = -np.sum(probability * np.log2(probability))
    return {k: float(v) for k, v in out.items()}


def f1_score(precision_, recall_):
    """F1 from the averaged precision and recall (Evaluator.py:257-263)."""
    return 2 * (precision_ * recall_) / (precision_ + recall_) if precision_ + recall_ != 0 else 0.0


def item_terms(URM_train):
    """Per-item NOVELTY and AVERAGE_POPULARITY terms from the column counts of the recommender's URM_train without explicit zeros
    (Novelty, metrics.py:552-559, 567-572; AveragePopularity, :601-611): -log2(pop / n_interactions) / n_items (0 where pop == 0)
    and pop / max(pop).  The counts are taken from the CSR rather than from a CSC copy (the same numbers, without transposing)."""
    train = sps.csr_matrix(URM_train)
    popularity = np.bincount(train.indices[train.data != 0], minlength=train.shape[1])
    novelty = np.zeros(len(popularity), np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        probability = popularity / popularity.sum()
        nonzero = probability != 0
        novelty[nonzero] = -np.log2(probability[nonzero]) / len(popularity)
        popularity_norm = np.ascontiguousarray(popularity / popularity.max(), dtype=np.float64)
    return novelty, popularity_norm


def users_to_evaluate(URM_test, min_ratings_per_user=1, ignore_items=None, ignore_users=None):
    """The evaluated users, ascending (int32; the reference iterates a set: order undefined there), and the mask of the users with
    enough test ratings: the copy of URM_test pruned of ignore_items decides who has `min_ratings_per_user` of them
    (Evaluator.py:124-138, 180-202), ignore_users are taken out afterwards (:204-211)."""
    pruned = sps.csr_matrix(URM_test).tocsc(copy=True)
    for item in np.asarray([] if ignore_items is None else ignore_items).astype(np.int64):
        pruned.data[pruned.indptr[item]:pruned.indptr[item + 1]] = 0
    pruned.eliminate_zeros()
    mask = np.ediff1d(sps.csr_matrix(pruned).indptr) >= min_ratings_per_user
    users = np.arange(pruned.shape[0])[mask]
    if ignore_users is not None:
        users = np.setdiff1d(users, np.array(ignore_users))
    return np.sort(users).astype(np.int32), mask


class EvaluatorHoldout_MI355X(N.Handle):
    """EvaluatorHoldout (Evaluator.py:382) on the device.  See the module docstring."""
    _PREFIX = "mi355rec_eval"

    EVALUATOR_NAME = "EvaluatorHoldout_MI355X"
    FUSED_BLOCK = 16384             # users per launch of the scorers that keep no n x n_items score buffer (candidate rows, item vector)

    def __init__(self, URM_test_list, cutoff_list, min_ratings_per_user=1, exclude_seen=True, diversity_object=None,
                 ignore_items=None, ignore_users=None, verbose=True):
        if isinstance(URM_test_list, list):
            raise ValueError("List of URM_test not supported")
        # (before anything touches the device; the range of the values is checked there, after the upload)
        diversity = None if diversity_object is None else diversity_matrix_of(diversity_object, URM_test_list.shape[1], check_values=False)
        self.metrics = METRICS if diversity is None else METRICS_WITH_DIVERSITY
        self.verbose = verbose
        self.ignore_items_flag = ignore_items is not None
        self.ignore_items_ID = np.array([]) if ignore_items is None else np.array(ignore_items)
        if self.ignore_items_flag:
            self._print("Ignoring {} Items".format(len(ignore_items)))
        self.cutoff_list = [int(c) for c in cutoff_list]
        if len(set(self.cutoff_list)) != len(self.cutoff_list) or min(self.cutoff_list) < 1:
            raise ValueError("cutoff_list must hold distinct positive cutoffs")
        self.max_cutoff = max(self.cutoff_list)
        self.min_ratings_per_user = min_ratings_per_user
        self.exclude_seen = exclude_seen
        self.URM_test = sps.csr_matrix(URM_test_list, copy=True)
        self.n_users, self.n_items = self.URM_test.shape
        self.width = min(self.max_cutoff, self.n_items)
        if diversity is not None and self.width > DIVERSITY_MAX_WIDTH:
            raise NotImplementedError("{}: DIVERSITY_SIMILARITY on lists of {} entries: at most {}".format(
                self.EVALUATOR_NAME, self.width, DIVERSITY_MAX_WIDTH))

        self.users_to_evaluate, mask = users_to_evaluate(self.URM_test, min_ratings_per_user, self.ignore_items_ID, ignore_users)
        if not np.all(mask):
            self._print("Ignoring {} ({:.2f}%) Users that have less than {} test interactions".format(
                np.sum(mask), 100 * np.sum(np.logical_not(mask)) / len(mask), min_ratings_per_user))
        if ignore_users is not None:
            self._print("Ignoring {} Users".format(len(ignore_users)))
        self.ignore_users_ID = np.array([]) if ignore_users is None else np.array(ignore_users)

        # relevant items and ratings: URM_test as passed (Evaluator.py:171, 279-291)
        indptr, indices = N.as_i32(self.URM_test.indptr), N.as_i32(self.URM_test.indices)
        relevance = np.ascontiguousarray(self.URM_test.data, dtype=np.float64)
        longest = int(np.max(np.ediff1d(indptr))) if self.n_users else 0
        log_len = max(self.width, longest, 1)
        log_table = np.log(np.arange(log_len, dtype=np.float32) + 2)                  # dcg (metrics.py:207-209)
        cutoffs = np.asarray(self.cutoff_list, dtype=np.int32)
        self._create(self.n_users, self.n_items, N.ptr(indptr), N.ptr(indices), N.ptr(relevance), N.ptr(cutoffs), len(cutoffs),
                     N.ptr(log_table), log_len)
        if diversity is not None:
            self._call("set_diversity", N.ptr(diversity), diversity.dtype.itemsize)
        self._per_user = self._per_user_diversity = None
        self.item_counts = None             # {cutoff: times each item was recommended within the cutoff}, last evaluation

    def _print(self, string):
        if self.verbose:
            print("{}: {}".format(self.EVALUATOR_NAME, string))

    def _block_size(self):
        """EvaluatorHoldout._run_evaluation_on_selected_users (Evaluator.py:406-408)."""
        return max(1, min(min(1000, int(1e8 / self.n_items)), len(self.users_to_evaluate)))

    def evaluateRecommender(self, recommender_object, block_size=None):
        """(results_dict, results_string) as Evaluator.evaluateRecommender (Evaluator.py:225-275).  `block_size` (users per block)
        defaults to the reference's rule; the result does not depend on it."""
        rec = recommender_object
        users = self.users_to_evaluate
        n_eval = len(users)
        started = time.time()
        if self.ignore_items_flag:
            rec.set_items_to_ignore(self.ignore_items_ID)
        try:
            novelty, popularity_norm = item_terms(rec.get_URM_train())
            if len(novelty) != self.n_items:
                raise ValueError("{}: URM_train has {} items, URM_test {}".format(self.EVALUATOR_NAME, len(novelty), self.n_items))
            if n_eval == 0:
                self._print("WARNING: No users had a sufficient number of relevant items")
                self._per_user = np.zeros((0, len(self.cutoff_list), N_VALUES))
                self._per_user_diversity = np.zeros((0, len(self.cutoff_list)))
                results = {c: {m: 0.0 for m in self.metrics} for c in self.cutoff_list}    # (Diversity_similarity.get_metric_value, metrics.py:683-688)
                return results, get_result_string(results)
            self._call("begin", N.ptr(novelty), N.ptr(popularity_norm), N.ptr(users), n_eval)
            self._run(rec, block_size)
            sums = np.zeros((len(self.cutoff_list), N_VALUES), np.float64)
            counts = np.zeros((len(self.cutoff_list), self.n_items), np.int32)
            self._call("finish", N.ptr(sums), N.ptr(counts))
            self._per_user_diversity = None
            diversity_sums = None
            if self.metrics is METRICS_WITH_DIVERSITY:
                diversity_sums = np.zeros(len(self.cutoff_list), np.float64)
                self._call("get_diversity", N.ptr(diversity_sums), None)
                if np.isnan(diversity_sums).any():          # (the validated matrix holds no NaN: a NaN sum means exactly a short list)
                    raise ZeroDivisionError("{}: a list of fewer than two items met a diversity_object (cutoffs {}): float division "
                                            "by zero in Diversity_similarity.add_recommendations".format(
                                                self.EVALUATOR_NAME, [c for c, s in zip(self.cutoff_list, diversity_sums) if np.isnan(s)]))
        finally:
            if self.ignore_items_flag:
                rec.reset_items_to_ignore()
        self._per_user = None
        self.item_counts = {cutoff: counts[c].copy() for c, cutoff in enumerate(self.cutoff_list)}
        results = {}
        for c, cutoff in enumerate(self.cutoff_list):
            mean = dict(zip(PER_USER, sums[c, :len(PER_USER)] / n_eval))
            row = {m: float(mean[m]) for m in PER_USER}
            row["F1"] = f1_score(row["PRECISION"], row["RECALL"])
            if diversity_sums is not None:
                row[DIVERSITY_SIMILARITY] = float(diversity_sums[c] / n_eval)
            row.update(population_metrics(counts[c], n_eval, cutoff, self.ignore_items_ID, self.n_users, len(self.ignore_users_ID),
                                          int(sums[c, N_VALUES - 1])))
            results[cutoff] = {m: row[m] for m in self.metrics}
        elapsed = time.time() - started
        self._print("Processed {} ( {:.2f}% ) in {:.2f} sec. Users per second: {:.0f}".format(
            n_eval, 100.0, elapsed, n_eval / max(elapsed, 1e-9)))
        sys.stdout.flush()
        return results, get_result_string(results)

    def _run(self, rec, block_size):
        """Every block of users through the fused path of the recommender's device scorer, or through its recommend()."""
        self._dispatch(rec, block_size, "rows")

    def _dispatch(self, rec, block_size, path):
        """path: what a device scorer ranks -- "rows" (entry point EVAL_ADD), "candidates" (EVAL_ADD_candidates) -- or None: every
        recommender through recommend()."""
        scorer = rec.device_scorer() if path and isinstance(rec, _ScoringMixin) else None
        large = scorer is not None and path in scorer.EVAL_LARGE_BLOCKS     # (no n x n_items score buffer bounds a launch)
        block = int(block_size) if block_size else (min(self.FUSED_BLOCK, len(self.users_to_evaluate)) if large else self._block_size())
        if scorer is None:
            self._run_lists(rec, block)
        else:
            self._run_fused(scorer, scorer.EVAL_ADD + ("" if path == "rows" else "_" + path), rec, block)

    def _run_fused(self, scorer, add, rec, block):
        allowed = allowed_items(rec, remove_custom_items_flag=self.ignore_items_flag)
        for start in range(0, len(self.users_to_evaluate), block):
            n = min(block, len(self.users_to_evaluate) - start)
            self._call(add, scorer._h, start, n, int(bool(self.exclude_seen)), N.ptr(allowed))

    def _put_list(self, table, r, items):
        """A user's list, checked, into row r of a block's -1 padded table."""
        items = np.asarray(items).ravel()
        if len(items) > self.width:
            raise ValueError("{}: a list of {} items for cutoff {}".format(self.EVALUATOR_NAME, len(items), self.max_cutoff))
        if len(items) and (items.min() < 0 or items.max() >= self.n_items):
            raise ValueError("{}: recommended item id outside [0, {})".format(self.EVALUATOR_NAME, self.n_items))
        table[r, :len(items)] = items

    def _run_lists(self, rec, block):
        users = self.users_to_evaluate
        for start in range(0, len(users), block):
            batch = users[start:start + block]
            lists = rec.recommend(batch, remove_seen_flag=self.exclude_seen, cutoff=self.max_cutoff, remove_top_pop_flag=False,
                                  remove_custom_items_flag=self.ignore_items_flag, return_scores=False)
            if len(lists) != len(batch):
                raise ValueError("{}: recommend() returned {} lists for {} users".format(self.EVALUATOR_NAME, len(lists), len(batch)))
            table = np.full((len(batch), self.width), -1, np.int32)
            for r, items in enumerate(lists):
                self._put_list(table, r, items)
            self._call("add_lists", start, len(batch), N.ptr(table))

    def per_user_values(self):
        """{cutoff: {metric: float64 array}} of the last evaluation, one entry per evaluated user in `users_to_evaluate` order:
        the per-user value the reference adds to each accumulated metric (Evaluator.py:334-345)."""
        if self._per_user is None:
            n_eval = len(self.users_to_evaluate)
            if n_eval == 0:
                self._per_user = np.zeros((0, len(self.cutoff_list), N_VALUES))
            else:
                out = np.zeros((n_eval, len(self.cutoff_list), N_VALUES), np.float64)
                self._call("get_per_user", N.ptr(out))
                self._per_user = out
        values = {cutoff: {m: self._per_user[:, c, v].copy() for v, m in enumerate(PER_USER)}
                  for c, cutoff in enumerate(self.cutoff_list)}
        if self.metrics is METRICS_WITH_DIVERSITY:
            if self._per_user_diversity is None:
                out = np.zeros((len(self.users_to_evaluate), len(self.cutoff_list)), np.float64)
                self._call("get_diversity", N.ptr(np.zeros(len(self.cutoff_list), np.float64)), N.ptr(out))
                self._per_user_diversity = out
            for c, cutoff in enumerate(self.cutoff_list):
                values[cutoff][DIVERSITY_SIMILARITY] = self._per_user_diversity[:, c].copy()
        return values


def items_to_rank(URM_test, URM_test_negative):
    """URM_items_to_rank of EvaluatorNegativeItemSample (Evaluator.py:484-486): per user, the columns with a non-zero stored value
    in URM_test or in URM_test_negative, each once, as a CSR of ones with the rows sorted by item id."""
    test, negative = sps.csr_matrix(URM_test), sps.csr_matrix(URM_test_negative)
    if test.shape != negative.shape:
        raise ValueError("URM_test is {}, URM_test_negative {}".format(test.shape, negative.shape))
    rows, cols = [], []
    for m in (test, negative):
        keep = m.data != 0
        rows.append(np.repeat(np.arange(m.shape[0]), np.ediff1d(m.indptr))[keep])
        cols.append(m.indices[keep])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    union = sps.csr_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=test.shape)
    union.sum_duplicates()
    union.sort_indices()
    union.data = np.ones(len(union.data), np.float64)
    return union


class EvaluatorNegativeItemSample_MI355X(EvaluatorHoldout_MI355X):
    """EvaluatorNegativeItemSample (Evaluator.py:455-539) on the device: the candidates of a user are its test items and the items
    of its row of URM_test_negative; its list is the `max_cutoff` best of them after the seen / ignored-item filters
    (BaseRecommender.py:131-222 with items_to_compute), ties towards the lower item id.  Users, relevance and every metric are the
    parent's.  Recommenders with a device scorer score and rank the candidates on the device (no score matrix); any other
    recommender is asked once per user, as the reference asks.  Candidate rows of more than 4096 items, or lists wider than that,
    send every recommender through recommend()."""

    EVALUATOR_NAME = "EvaluatorNegativeItemSample_MI355X"

    def __init__(self, URM_test_list, URM_test_negative, cutoff_list, min_ratings_per_user=1, exclude_seen=True, diversity_object=None,
                 ignore_items=None, ignore_users=None, verbose=True):
        if isinstance(URM_test_list, list):
            raise ValueError("List of URM_test not supported")
        if tuple(URM_test_list.shape) != tuple(URM_test_negative.shape):
            raise ValueError("URM_test is {}, URM_test_negative {}".format(URM_test_list.shape, URM_test_negative.shape))
        super().__init__(URM_test_list, cutoff_list, min_ratings_per_user=min_ratings_per_user, exclude_seen=exclude_seen,
                         diversity_object=diversity_object, ignore_items=ignore_items, ignore_users=ignore_users, verbose=verbose)
        self.URM_items_to_rank = items_to_rank(self.URM_test, URM_test_negative)       # (URM_test as passed: not pruned of ignore_items)
        indptr, indices = N.as_i32(self.URM_items_to_rank.indptr), N.as_i32(self.URM_items_to_rank.indices)
        try:
            self._call("set_candidates", N.ptr(indptr), N.ptr(indices))
            self.candidates_on_device = True
        except NotImplementedError as unsupported:
            self.candidates_on_device = False
            self._print("every recommender goes through recommend(), one user at a time: {}".format(unsupported))

    def _candidates(self, user):
        rows = self.URM_items_to_rank
        return rows.indices[rows.indptr[user]:rows.indptr[user + 1]]

    def _run(self, rec, block_size):
        self._dispatch(rec, block_size, "candidates" if self.candidates_on_device else None)

    def _run_lists(self, rec, block):
        """Evaluator.py:519-530: recommend() per user with the user's candidates as items_to_compute; the lists of a block of users go
        up together."""
        users = self.users_to_evaluate
        for start in range(0, len(users), block):
            batch = users[start:start + block]
            table = np.full((len(batch), self.width), -1, np.int32)
            for r, user in enumerate(batch):
                lists = rec.recommend(np.atleast_1d(user), remove_seen_flag=self.exclude_seen, cutoff=self.max_cutoff,
                                      remove_top_pop_flag=False, items_to_compute=self._candidates(user),
                                      remove_custom_items_flag=self.ignore_items_flag, return_scores=False)
                if len(lists) != 1:
                    raise ValueError("{}: recommend() returned {} lists for one user".format(self.EVALUATOR_NAME, len(lists)))
                self._put_list(table, r, lists[0])
            self._call("add_lists", start, len(batch), N.ptr(table))
