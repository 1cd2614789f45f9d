"""Every stream of tests/mf_stream_cases.py contains what its name claims (no GPU).

batch_book() restates the bookkeeping of the in-LDS schedule's sort kernel (csrc/mf_schedule.cuh, mf_sched_sort_body) in NumPy: the
runs of a mini-batch in (row, stream) order, which runs are wide, which are absorbed by their sample's user task, which lone users
share a pair task, and the header slots the mini-batch uses.  The cases are then asserted run length by run length, and replayed
through the CPU oracle.
"""
import numpy as np
import pytest
import scipy.sparse as sps

import mf_stream_cases as S
from oracle import oracle as O

GROUPS = (1, 2, 4)
FAST_MAX_BATCHES, QTASK_OFF_MAX = 256, 31


def wide_now(length, group):
    return length > max(2 * group, 3)


def wide_parent(length, group):
    """the rule before list_is_wide(): longer than two rounds of one wavefront, whatever the group"""
    return length > 2 * group


def batch_book(u, i, j, n_users, group, fuse, wide=wide_now):
    """One mini-batch (j None: FunkSVD).  Incidence q = sample * per + role; the sort is stable on the row.  Returns the runs as
    (row, start, length) in sorted order and, per run, wide / absorbed / pair flags; `used` = the header slots the sort kernel
    hands out: 4 per wide run, 1 per other run with a header of its own."""
    per = 2 if j is None else 3
    cols = [np.asarray(u, np.int64), n_users + np.asarray(i, np.int64)] + ([] if j is None else [n_users + np.asarray(j, np.int64)])
    rows = np.stack(cols, 1).reshape(-1)
    m = len(rows)
    order = np.argsort(rows, kind="stable")
    srt = rows[order]
    starts = np.flatnonzero(np.r_[True, srt[1:] != srt[:-1]])
    lens = np.diff(np.r_[starts, m])
    single = np.zeros(m, bool)
    single[order[starts[lens == 1]]] = True
    run_of = np.repeat(np.arange(len(starts)), lens)

    def lone_user(q):
        return q < m and srt[q] < n_users and lens[run_of[q]] == 1

    def paired(q):
        q0 = q - q % group
        return bool(fuse) and group >= 2 and all(lone_user(q0 + e) for e in range(group))

    is_wide = np.array([wide(int(n), group) for n in lens])
    absorbed = np.zeros(len(starts), bool)
    pair = np.zeros(len(starts), bool)
    for t, (start, n) in enumerate(zip(starts, lens)):
        if n != 1:
            continue
        inc = order[start]
        absorbed[t] = bool(fuse) and inc % per != 0 and single[inc - inc % per]
        pair[t] = paired(int(start))
    no_header = absorbed | (pair & (starts % group != 0))
    used = 4 * int(is_wide.sum()) + int((~is_wide & ~no_header).sum())
    return dict(rows=srt[starts], starts=starts, lens=lens, wide=is_wide, absorbed=absorbed, pair=pair, used=used, per=per, m=m,
                single=single, order=order)


def batches(u, i, third, B, algorithm):
    for a in range(0, len(u), B):
        yield u[a:a + B], i[a:a + B], third[a:a + B] if algorithm == "MF_BPR" else None


def run_lengths(book, n_users, items):
    sel = (book["rows"] >= n_users) if items else (book["rows"] < n_users)
    return sorted(book["lens"][sel].tolist())


ALL = [(case, algorithm, shape, group) for algorithm in S.ALGORITHMS for case in S.cases_of(algorithm) for shape in S.SHAPES for group in GROUPS]


def test_the_case_list():
    assert set(S.cases_of("MF_BPR")) == {"all_threes", "one_three_rest_single", "straddle", "offsets", "one_row_everywhere", "partial_tail",
                                         "partial_tail_one_sample", "every_batch", "roles_mixed"}
    assert set(S.cases_of("FUNK_SVD")) == set(S.cases_of("MF_BPR")) - {"roles_mixed"}
    assert S.SHAPES == ((97, 60), (96, 32)) and [(a + b) % 32 for a, b in S.SHAPES] == [29, 0]       # a partial last bit-row word | whole words


@pytest.mark.parametrize("case,algorithm,shape,group", ALL)
def test_builders_are_seeded_and_no_mini_batch_overruns_its_header_slots(case, algorithm, shape, group):
    a, b = S.build(case, *shape, group, algorithm), S.build(case, *shape, group, algorithm)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    u, i, third, B = a
    for fuse in ((True, False) if algorithm == "MF_BPR" else (False,)):
        for ub, ib, jb in batches(u, i, third, B, algorithm):
            book = batch_book(ub, ib, jb, shape[0], group, fuse)
            assert book["used"] <= book["per"] * B and book["lens"].sum() == book["m"], (fuse, book["used"])


@pytest.mark.parametrize("algorithm", S.ALGORITHMS)
@pytest.mark.parametrize("shape", S.SHAPES)
@pytest.mark.parametrize("group", GROUPS)
def test_all_threes(algorithm, shape, group):
    u, i, third, B = S.build("all_threes", *shape, group, algorithm)
    assert B == 48 == len(u) and len(set(zip(u.tolist(), i.tolist()))) == 48
    bpr = algorithm == "MF_BPR"
    book = batch_book(u, i, third if bpr else None, shape[0], 1, False, wide_parent)
    assert run_lengths(book, shape[0], False) == [3] * 16 and run_lengths(book, shape[0], True) == [3] * (32 if bpr else 16)
    assert sorted(set(i.tolist())) == list(range(16))
    # the instances with one sample in flight: the parent's rule needs 4 slots per run of 3, the mini-batch has 3
    tpb = book["per"] * B
    assert book["used"] == 4 * len(book["lens"]) > tpb
    for fuse in (True, False):
        assert batch_book(u, i, third if bpr else None, shape[0], 1, fuse, wide_parent)["used"] > tpb
        assert batch_book(u, i, third if bpr else None, shape[0], 1, fuse)["used"] == len(book["lens"]) <= tpb


@pytest.mark.parametrize("algorithm", S.ALGORITHMS)
@pytest.mark.parametrize("shape", S.SHAPES)
@pytest.mark.parametrize("group", GROUPS)
def test_one_three_rest_single(algorithm, shape, group):
    u, i, third, B = S.build("one_three_rest_single", *shape, group, algorithm)
    assert B == 33 == len(u) and i[0] == i[1] == i[2] and (i[3:] != i[0]).all()
    bpr = algorithm == "MF_BPR"
    j = third if bpr else None
    book = batch_book(u, i, j, shape[0], 1, False, wide_parent)
    assert run_lengths(book, shape[0], False) == [1] * 33
    items = run_lengths(book, shape[0], True)
    if bpr:
        # 66 item incidences on n_items rows in runs of 1 and 3 only, as few threes as that allows (3 on 60 items, 17 on 32)
        assert (j != i[0]).all() and set(items) == {1, 3} and items.count(3) == max(1, -(-(66 - shape[1]) // 2))
    else:
        assert items == [1] * 30 + [3]
    tpb = book["per"] * B
    # one sample in flight, one task per row (FunkSVD always; BPR under MI355REC_MF_NO_FUSE): a header too many per run of 3
    assert book["used"] == tpb + items.count(3) > tpb
    assert batch_book(u, i, j, shape[0], 1, False)["used"] == len(book["lens"]) <= tpb
    if bpr:
        # fused, every once-touched item is absorbed by its lone user's task: slack for the 3 threes on 60 items (33 + 12 slots), not
        # for the 17 on 32 items (33 + 68 of 99) -- the default schedule overran there, too
        assert (batch_book(u, i, j, shape[0], 1, True, wide_parent)["used"] > tpb) == (shape[1] == 32)
        assert batch_book(u, i, j, shape[0], 1, True)["used"] <= tpb


@pytest.mark.parametrize("algorithm", S.ALGORITHMS)
@pytest.mark.parametrize("shape", S.SHAPES)
@pytest.mark.parametrize("group", GROUPS)
def test_straddle(algorithm, shape, group):
    u, i, third, B = S.build("straddle", *shape, group, algorithm)
    g = group
    want = [2 * g, 2 * g + 1, 4 * g - 1, 4 * g, 4 * g + 1, 8 * g, 8 * g + 1]
    assert S.straddle_lengths(g) == want and len(u) == B == sum(want) // (2 if algorithm == "MF_BPR" else 1)
    book = batch_book(u, i, third if algorithm == "MF_BPR" else None, shape[0], g, algorithm == "MF_BPR")
    assert run_lengths(book, shape[0], True) == sorted(want)
    users = run_lengths(book, shape[0], False)
    assert users == [1] * B if B <= shape[0] else (max(users) == 2 and len(users) == shape[0])
    wide = dict(zip(book["lens"][book["rows"] >= shape[0]].tolist(), book["wide"][book["rows"] >= shape[0]].tolist()))
    # both sides of the wide threshold; wide lists whose last quarters stay empty (fewer than 3 g + 1 samples), hold one sample, run twice
    assert wide == {n: n > max(2 * g, 3) for n in want} and not wide[2 * g] and wide[4 * g]
    assert any(w and n <= 3 * g for n, w in wide.items()) == (g > 1) and wide[4 * g + 1] and wide[8 * g + 1]


@pytest.mark.parametrize("algorithm", S.ALGORITHMS)
@pytest.mark.parametrize("shape", S.SHAPES)
@pytest.mark.parametrize("group", GROUPS)
def test_offsets_and_one_row_everywhere(algorithm, shape, group):
    bpr = algorithm == "MF_BPR"
    u, i, third, B = S.build("offsets", *shape, group, algorithm)
    book = batch_book(u, i, third if bpr else None, shape[0], group, bpr)
    items = run_lengths(book, shape[0], True)
    assert B == 96 == len(u) and run_lengths(book, shape[0], False) == [96]
    assert {QTASK_OFF_MAX, QTASK_OFF_MAX + 1, QTASK_OFF_MAX + 2} <= set(items) and (bpr or items == [31, 32, 33])
    u, i, third, B = S.build("one_row_everywhere", *shape, group, algorithm)
    book = batch_book(u, i, third if bpr else None, shape[0], group, bpr)
    assert B == 64 == len(u) and run_lengths(book, shape[0], False) == [64]
    assert bpr or run_lengths(book, shape[0], True) == [64]


@pytest.mark.parametrize("algorithm", S.ALGORITHMS)
@pytest.mark.parametrize("shape", S.SHAPES)
def test_partial_tail_and_every_batch(algorithm, shape):
    u, _, _, B = S.build("partial_tail", *shape, 1, algorithm)
    assert B == 16 and len(u) == 3 * B + 1
    u, _, _, B = S.build("partial_tail_one_sample", *shape, 1, algorithm)
    assert B == 16 and len(u) == 1
    u, i, third, B = S.build("every_batch", *shape, 1, algorithm)
    n_batches = len(u) // B
    assert B == 4 and len(u) == 4 * n_batches and n_batches == 300 > FAST_MAX_BATCHES
    touched = {}
    for b, (ub, ib, jb) in enumerate(batches(u, i, third, B, algorithm)):
        for row in batch_book(ub, ib, jb, shape[0], 1, False)["rows"].tolist():
            touched.setdefault(row, []).append(b)
    want = S.every_batch_rows(*shape)
    assert sorted(want) == [shape[0] - 1, shape[0], shape[0] + shape[1] - 1]
    assert want[shape[0] - 1] == list(range(300)) and want[shape[0]] == [0, 299] and want[shape[0] + shape[1] - 1] == [255, 256]
    for row, where in want.items():
        assert touched[row] == where, row


@pytest.mark.parametrize("shape", S.SHAPES)
@pytest.mark.parametrize("group", GROUPS)
def test_roles_mixed(shape, group):
    u, i, j, B = S.build("roles_mixed", *shape, group, "MF_BPR")
    n_users = shape[0]
    assert len(u) == B
    book = batch_book(u, i, j, n_users, group, True)
    assert set(i.tolist()) & set(j.tolist()), "an item that is positive in one sample and negative in another"
    count_u, count_item = np.bincount(u, minlength=n_users), np.bincount(np.r_[i, j], minlength=shape[1])
    lone = count_u[u] == 1
    assert (lone & (count_item[i] == 1) & (count_item[j] == 1)).any(), "a fully fused sample"
    assert (lone & (count_item[i] > 1)).any(), "a lone user whose positive item is shared"
    fused_both = [t for t in np.flatnonzero(book["absorbed"])]
    assert len(fused_both) >= 2 and not book["wide"].any()
    if group == 1:
        assert not book["pair"].any()
        return
    user_pos = np.flatnonzero(np.repeat(book["rows"], book["lens"]) < n_users)
    lone_pos = set(np.repeat(book["starts"], 1)[(book["lens"] == 1) & (book["rows"] < n_users)].tolist())
    blocks = {}
    for q in user_pos.tolist():
        blocks.setdefault(q // group, []).append(q in lone_pos)
    whole = [b for b, flags in blocks.items() if len(flags) == group and all(flags)]
    broken = [b for b, flags in blocks.items() if any(flags) and not all(flags)]
    assert whole and broken, (whole, broken)
    # consecutive user ids fill the whole blocks; their runs are the pair tasks, one header per block
    paired_starts = book["starts"][book["pair"]]
    assert sorted(set((paired_starts // group).tolist())) == sorted(whole) and len(paired_starts) == group * len(whole)
    first = book["rows"][book["pair"]].reshape(-1, group)
    assert (np.diff(first, axis=1) == 1).all()


@pytest.mark.parametrize("case,algorithm,shape,group", ALL)
def test_the_oracle_replays_every_case_to_finite_factors(case, algorithm, shape, group):
    u, i, third, B = S.build(case, *shape, group, algorithm)
    X = sps.random(*shape, density=0.2, format="csr", random_state=3, dtype=np.float64)
    X.data[:] = 1.0 + np.floor(X.data * 5.0).clip(0, 4)
    orc = O.OracleMF(X, n_factors=6, algorithm_name=algorithm, batch_size=B, random_seed=9, sgd_mode="adam", learning_rate=0.05,
                     user_reg=0.002, item_reg=0.003, positive_reg=0.003, negative_reg=0.004, bias_reg=0.005,
                     use_bias=algorithm == "FUNK_SVD" and case in S.FUNK_WITH_BIAS)
    start = orc.get_USER_factors().copy()
    if algorithm == "MF_BPR":
        orc.replay(u, i, j=third)
    else:
        orc.replay(u, i, rating=third)
    U, V = orc.get_USER_factors(), orc.get_ITEM_factors()
    assert np.isfinite(U).all() and np.isfinite(V).all() and np.isfinite(orc.get_USER_bias()).all() and np.isfinite(orc.get_ITEM_bias()).all()
    assert np.isfinite(float(orc.get_GLOBAL_bias())) and (U != start).any()
