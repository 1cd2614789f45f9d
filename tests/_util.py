"""Shared helpers of the test-suite (comparators, fixture loading)."""
import json
import os

import numpy as np
import scipy.sparse as sps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    cases = json.loads(str(z["cases"]))
    return z, cases


def unpack_csr(z, prefix):
    shape = tuple(int(x) for x in z[prefix + "_shape"])
    return sps.csr_matrix((z[prefix + "_data"], z[prefix + "_indices"], z[prefix + "_indptr"]), shape=shape)


def rel_err(a, b):
    """max |a-b| / max(|b|) -- the '1e-5 relative on float32 factor matrices / similarity values' of north_star."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    return np.abs(a - b).max() / scale


def elementwise_close(a, b, rtol, atol_frac=1e-6):
    """|a-b| <= rtol*|b| + atol_frac*max|b| everywhere."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    tol = rtol * np.abs(b) + atol_frac * np.abs(b).max()
    bad = np.abs(a - b) > tol
    return not bad.any(), (np.abs(a - b) - tol).max()


def check_topk_against_dense(idx, val, dense_col, topK, rtol=1e-5):
    """Tie-aware top-K check of ONE column.

    idx/val : device (or oracle) output, -1 padded, value-descending
    dense_col: the full normalised column (float64) from the oracle
    Rule (SURVEY section 7 hard part 4): with t = K-th largest value of the column (zeros compete, then are dropped),
    every cell strictly above t (beyond tolerance) must be present, nothing below t (beyond tolerance) may be
    present, the emitted values must match the oracle's values for the emitted indices, order must be
    non-increasing, and no zero may be emitted.
    """
    n = len(dense_col)
    K = min(topK, n)
    got = idx[idx >= 0]
    got_val = val[:len(got)]
    assert (idx[len(got):] == -1).all(), "padding must be trailing"
    assert len(np.unique(got)) == len(got), "duplicate neighbour"
    scale = max(np.abs(dense_col).max(), 1e-30)
    tol = rtol * scale
    order = np.sort(dense_col)[::-1]
    t = order[K - 1]
    must = np.flatnonzero((dense_col > t + tol) & (dense_col != 0))
    assert np.isin(must, got).all(), "a cell strictly above the K-th value is missing"
    allowed = dense_col[got]
    assert (allowed >= t - tol).all(), "a cell strictly below the K-th value was emitted"
    assert (allowed != 0).all(), "a zero similarity was emitted"
    expected_count = min(K, int(((dense_col >= t - tol) & (dense_col != 0)).sum()))
    strict_count = int(((dense_col > t + tol) & (dense_col != 0)).sum())
    assert strict_count <= len(got) <= max(expected_count, strict_count)
    np.testing.assert_allclose(got_val, allowed, rtol=rtol, atol=tol)
    assert (np.diff(got_val) <= tol).all(), "values must be non-increasing"


# Relative error a cell of an UN-NORMALISED build may show against a float64 oracle that was given the same float32 input values, one
# 2^-24 (half a float32 ulp) per float32 rounding on the way -- derived from the operations, not measured:
#   builder slabs (Compute_Similarity_MI355X.compute_slabs): the float64 (or exact fixed-point) column sum is stored as float32 -- 1;
#   walk rows (graph_based._fit_walk, W_rowwise): that store, the multiplication by row_factor and the cast to float32 -- 3 (the
#     multiplication runs in float64 today and then costs 2^-53; its slot is kept so that the bound also covers a float32 product).
# The float64 sum itself adds n * 2^-53 for n products of one sign, below 2^-40 for the 8 192 users a test column may have.
# On the int64 fixed-point accumulator the gate of create_fixed_point (sim.hip) promises a worst-case 1e-6 on top of that.
F32_ROUNDING = 2.0 ** -24
F64_SUM_SLACK = 2.0 ** -40
FIXED_POINT_PROMISE = 1e-6


def per_cell_bound(accumulator_kind, f32_roundings):
    """Relative bound of one emitted cell: `f32_roundings` float32 roundings, plus the fixed-point gate's promise where it applies."""
    assert accumulator_kind in ("uint32", "int32-exact", "int64-fixed", "float64")
    return f32_roundings * F32_ROUNDING + F64_SUM_SLACK + (FIXED_POINT_PROMISE if accumulator_kind == "int64-fixed" else 0.0)


def check_topk_per_cell(idx, val, dense_col, topK, rtol):
    """check_topk_against_dense with every tolerance taken relative to the CELL instead of to the column's largest value -- for raw sums,
    whose cells span many decades (a bound relative to the maximum lets a cell a thousand times smaller be entirely wrong).

    Same membership rule: with t = K-th largest value of the column (zeros compete, then are dropped), a cell x is in the tie class
    of the cut when |x - t| <= rtol * max(|x|, |t|); every non-zero cell above the class must be present, nothing below it may be,
    no zero may be emitted, the count follows, and the order is non-increasing up to the same relative band.  Every emitted value must
    lie within rtol * |x| of the oracle's value x of its own cell.  Returns the largest relative error of the emitted values."""
    dense_col = np.asarray(dense_col, dtype=np.float64)
    n = len(dense_col)
    K = min(topK, n)
    got = idx[idx >= 0]
    got_val = np.asarray(val[:len(got)], dtype=np.float64)
    assert (idx[len(got):] == -1).all(), "padding must be trailing"
    assert len(np.unique(got)) == len(got), "duplicate neighbour"
    t = np.sort(dense_col)[::-1][K - 1]
    band = rtol * np.maximum(np.abs(dense_col), abs(t))
    above = (dense_col - t > band) & (dense_col != 0)
    not_below = (dense_col - t >= -band) & (dense_col != 0)
    assert np.isin(np.flatnonzero(above), got).all(), "a cell strictly above the K-th value is missing"
    assert (dense_col[got] != 0).all(), "a zero similarity was emitted"
    assert not_below[got].all(), "a cell strictly below the K-th value was emitted"
    strict_count = int(above.sum())
    assert strict_count <= len(got) <= max(min(K, int(not_below.sum())), strict_count)
    want = dense_col[got]
    err = np.abs(got_val - want) / np.abs(want) if len(got) else np.zeros(0)
    worst = float(err.max()) if len(got) else 0.0
    assert worst <= rtol, "cell %d: %.9g against %.9g, relative error %.3g > %.3g" % (
        got[int(err.argmax())], got_val[int(err.argmax())], want[int(err.argmax())], worst, rtol)
    assert (np.diff(got_val) <= 2 * rtol * np.abs(got_val[:-1])).all(), "values must be non-increasing"
    return worst


def csr_columns_as_slabs(W, topK):
    """csr/csc matrix with <= topK entries per column -> (idx, val) slabs sorted by descending value."""
    W = sps.csc_matrix(W)
    n = W.shape[1]
    idx = -np.ones((n, topK), np.int32); val = np.zeros((n, topK), np.float32)
    for c in range(n):
        s, e = W.indptr[c], W.indptr[c + 1]
        o = np.argsort(-W.data[s:e], kind="stable")
        idx[c, :e - s] = W.indices[s:e][o]; val[c, :e - s] = W.data[s:e][o]
    return idx, val


def block_pair_create_refusals(prefix, width_noun, nmf=False):
    """Every refusal of mi355rec_<prefix>_create (the PureSVD and NMF handles share them), word for word.  All of them come before the
    device is touched.  Returns the messages seen, in the order of the checks."""
    import ctypes as C
    from recsys2019_deeplearning_evaluation_amd import _native as N
    lib = N.load()
    create = getattr(lib, "mi355rec_%s_create" % prefix)
    # 3 users x 4 items: [[1, 0, 0, 2], [0, 0, 0, 0], [0, 3, 0, 0]]
    good = dict(n_users=3, n_items=4, width=2, row_ptr=[0, 2, 2, 3], row_idx=[0, 3, 1], row_val=[1, 2, 3], col_ptr=[0, 1, 2, 2, 3], col_idx=[0, 2, 0],
                col_val=[1, 3, 2])
    big = 128 * 65535 + 1

    def refused(out=True, **changes):
        a = dict(good, **changes)
        arrays = [None if a[name] is None else (N.as_f32 if name.endswith("val") else N.as_i32)(a[name])
                  for name in ("row_ptr", "row_idx", "row_val", "col_ptr", "col_idx", "col_val")]
        h = C.c_void_p()
        rc = create(C.byref(h) if out else None, a["n_users"], a["n_items"], a["width"], *[N.ptr(x) for x in arrays])
        assert rc == N.E_INVALID and not h.value, changes
        return lib.mi355rec_last_error().decode()

    seen = [refused(out=False), refused(row_ptr=None), refused(col_ptr=None), refused(row_val=None), refused(col_idx=None)]
    assert seen == ["NULL argument"] * 5
    seen += [refused(n_users=0), refused(n_items=-1)]
    assert seen[-2:] == ["empty URM (0 x 4)", "empty URM (3 x -1)"]
    seen += [refused(width=w) for w in (0, -3, 4097)]
    assert seen[-3:] == ["%s = %d outside [1, 4096]" % (width_noun, w) for w in (0, -3, 4097)]
    seen.append(refused(col_ptr=[0, 1, 2, 2, 2]))
    assert seen[-1] == "the two layouts hold 3 and 2 cells"
    seen.append(refused(n_users=big, row_ptr=np.zeros(big + 1, np.int32), col_ptr=[0, 0, 0, 0, 0], row_idx=None, col_idx=None, row_val=None, col_val=None))
    assert seen[-1] == "more than 8 M rows on a side"
    seen += [refused(row_ptr=[1, 2, 2, 3]), refused(row_ptr=[0, 2, 1, 3]), refused(col_ptr=[0, 1, 2, 4, 3]), refused(row_idx=[0, 4, 1]),
             refused(col_idx=[0, 2, -1]), refused(col_idx=[3, 2, 0])]
    assert seen[-6:] == ["row pointers do not start at 0", "row pointers decrease at 1", "row pointers decrease at 3", "index 4 outside [0, 4)",
                         "index -1 outside [0, 3)", "index 3 outside [0, 3)"]
    if nmf:
        seen += [refused(row_val=[1, -1, 3]), refused(row_val=[1, 2, -0.25], col_val=[1, -0.25, 2])]
        assert seen[-2:] == ["negative value -1 in the URM", "negative value -0.25 in the URM"]
    return seen
