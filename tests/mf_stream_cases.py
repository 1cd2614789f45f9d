"""Sample streams built for the branches of the BPR-MF / FunkSVD mini-batch schedule (csrc/mf_schedule.cuh), pure NumPy.

The parity tests of test_mf_gpu.py replay streams the reference sampler drew: users touched once per mini-batch, short item lists.
The schedule's branches depend on the RUN LENGTHS inside a mini-batch (a run = the incidences of one row in one mini-batch): lists
split over a workgroup and their empty quarters, fused sample tasks and absorbed rows, pair tasks in aligned blocks, the saturated
run offset in qtask[], partial bit-row words, schedule parts of 256 mini-batches.  Every builder here makes a stream that reaches
named branches on purpose; tests/test_mf_stream_cases_spec.py checks on the CPU that it does, tests/test_mf_streams_gpu.py replays
it on the device and through the oracle.

build(case, n_users, n_items, group, algorithm) -> (u, i, third, batch_size): int32 users and items, `third` the int32 negative
items (algorithm "MF_BPR", i != j in every sample) or the float64 ratings ("FUNK_SVD": 1..5, 0 for a negative sample).  `group` =
samples a wavefront of the kernel instance works on at a time (mf_plan.h, samples_in_flight): 1, 2 or 4.  Same arguments, same
stream.
"""
import numpy as np

# users x items: 157 rows = 4 whole bit-row words and a partial fifth | 128 rows = 4 whole words
SHAPES = ((97, 60), (96, 32))
ALGORITHMS = ("MF_BPR", "FUNK_SVD")
SEED = 20240611


def _rng(case, n_users, n_items, group, algorithm):
    return np.random.default_rng([SEED, sorted(CASES).index(case), n_users, n_items, group, ALGORITHMS.index(algorithm)])


def _ratings(rng, n):
    """stored ratings 1..5, and about one sample in five a FunkSVD negative (rating 0)"""
    r = rng.integers(1, 6, n).astype(np.float64)
    r[rng.random(n) < 0.2] = 0.0
    return r


def _finish(rng, algorithm, u, i, j, batch_size, shuffle=True):
    """arrays of the right types; the samples of a one-batch stream in a seeded order, so that runs interleave in stream order"""
    u, i = np.asarray(u, np.int64), np.asarray(i, np.int64)
    order = rng.permutation(len(u)) if shuffle else np.arange(len(u))
    if algorithm == "MF_BPR":
        j = np.asarray(j, np.int64)
        assert (i != j).all()
        return u[order].astype(np.int32), i[order].astype(np.int32), j[order].astype(np.int32), batch_size
    return u[order].astype(np.int32), i[order].astype(np.int32), _ratings(rng, len(u)), batch_size


def _other_items(rng, n, n_items, avoid, exclude=()):
    """n items drawn from those not in `exclude`, each different from `avoid` at its position"""
    pool = np.setdiff1d(np.arange(n_items), np.asarray(exclude, np.int64))
    out = pool[rng.integers(0, len(pool), n)]
    clash = out == avoid
    while clash.any():
        out[clash] = pool[rng.integers(0, len(pool), int(clash.sum()))]
        clash = out == avoid
    return out


def _pair_up(rng, items):
    """an even list of item incidences, no item in more than half of them, as (i, j) columns with i != j: incidence t of the sorted
    list goes with incidence t + half; which of the two is the positive item is drawn"""
    items = np.sort(np.asarray(items, np.int64))
    half = len(items) // 2
    assert len(items) == 2 * half and np.bincount(items).max() <= half
    a, b = items[:half], items[half:]
    flip = rng.random(half) < 0.5
    return np.where(flip, b, a), np.where(flip, a, b)


def all_threes(n_users, n_items, group, algorithm, rng):
    """B = 48, a full mini-batch: 16 users and 16 items, each in exactly three samples, all (user, item) pairs distinct
    (item = (user + s) % 16, s = 0..2); BPR: the negatives are 16 further items, three samples each (16 + (user + s + 1) % 16)."""
    user = np.tile(np.arange(16), 3)
    s = np.repeat(np.arange(3), 16)
    return _finish(rng, algorithm, user, (user + s) % 16, 16 + (user + s + 1) % 16, 48)


def one_three_rest_single(n_users, n_items, group, algorithm, rng):
    """B = 33: one item is the (positive) item of samples 0..2, every user is touched once.  FunkSVD: every other item once, too.
    BPR's 66 item incidences do not fit that many rows: the other items are touched once wherever the shape has rows for it and
    three times otherwise -- runs of 1 and 3 only, with as few threes as the shape allows."""
    B = 33
    user = rng.permutation(n_users)[:B]
    if algorithm == "FUNK_SVD":
        rest = rng.permutation(np.arange(1, n_items))[:B - 3]
        return _finish(rng, algorithm, user, np.concatenate([[0, 0, 0], rest]), None, B, shuffle=False)
    threes = max(1, -(-(2 * B - n_items) // 2))         # 3 a + b = 66 incidences on a + b <= n_items rows
    singles = 2 * B - 3 * threes
    ids = rng.permutation(np.arange(1, n_items))
    others = np.concatenate([np.repeat(ids[:threes - 1], 3), ids[threes - 1:threes - 1 + singles]])
    for _ in range(10000):
        p = rng.permutation(others)
        i, j = np.concatenate([[0, 0, 0], p[:B - 3]]), p[B - 3:]
        if (i != j).all():
            return _finish(rng, algorithm, user, i, j, B, shuffle=False)
    raise AssertionError("no arrangement with i != j")


def straddle_lengths(group):
    g = group
    return [2 * g, 2 * g + 1, 4 * g - 1, 4 * g, 4 * g + 1, 8 * g, 8 * g + 1]


def straddle(n_users, n_items, group, algorithm, rng):
    """One mini-batch whose item runs have the lengths 2g, 2g+1 (the wide threshold), 4g-1, 4g, 4g+1 (quarters of a wide list that
    stay empty or hold one sample) and 8g, 8g+1 (a second round of every quarter): items 0..6, 32 g + 2 incidences.  FunkSVD: that
    many samples; BPR: half as many, a run's incidences in either role.  All users are distinct where the shape has as many users
    as the mini-batch has samples (FunkSVD at g = 4 needs 130: the users go round, none more than twice)."""
    items = np.repeat(np.arange(7), straddle_lengths(group))
    if algorithm == "MF_BPR":
        i, j = _pair_up(rng, items)
    else:
        i, j = items, None
    B = len(i)
    user = rng.permutation(n_users)[np.arange(B) % n_users]
    return _finish(rng, algorithm, user, i, j, B)


def offsets(n_users, n_items, group, algorithm, rng):
    """B = 96: item runs of 31, 32 and 33 (offsets within a run up to and past QTASK_OFF_MAX = 31, where qtask[] saturates) and one
    user in every sample (a run of 96).  BPR: the negatives go round the other items."""
    i = np.repeat(np.arange(3), [31, 32, 33])
    j = 3 + np.arange(96) % (n_items - 3)
    return _finish(rng, algorithm, np.full(96, n_users // 2), i, j, 96)


def one_row_everywhere(n_users, n_items, group, algorithm, rng):
    """B = 64: the same user in every sample; FunkSVD: the same item in every sample, too (two runs of 64 and nothing else)"""
    user = np.full(64, n_users - 2)
    if algorithm == "FUNK_SVD":
        return _finish(rng, algorithm, user, np.full(64, n_items // 2), None, 64)
    i = rng.integers(0, n_items, 64)
    return _finish(rng, algorithm, user, i, _other_items(rng, 64, n_items, i), 64)


def _random_stream(n, n_users, n_items, algorithm, rng, batch_size):
    i = rng.integers(0, n_items, n)
    return _finish(rng, algorithm, rng.integers(0, n_users, n), i, _other_items(rng, n, n_items, i), batch_size, shuffle=False)


def partial_tail(n_users, n_items, group, algorithm, rng):
    """3 B + 1 samples with B = 16: the last mini-batch holds one sample (and is still averaged over B)"""
    return _random_stream(3 * 16 + 1, n_users, n_items, algorithm, rng, 16)


def partial_tail_one_sample(n_users, n_items, group, algorithm, rng):
    """a stream of a single sample with B = 16"""
    return _random_stream(1, n_users, n_items, algorithm, rng, 16)


EVERY_BATCH_BATCHES = 300


def every_batch_rows(n_users, n_items):
    """(row as the schedule numbers it: users, then items) -> the mini-batches that touch it"""
    return {n_users - 1: list(range(EVERY_BATCH_BATCHES)), n_users + 0: [0, EVERY_BATCH_BATCHES - 1], n_users + n_items - 1: [255, 256]}


def every_batch(n_users, n_items, group, algorithm, rng):
    """300 mini-batches of B = 4 (more than FAST_MAX_BATCHES = 256: two schedule parts).  User n_users - 1 is touched in every
    mini-batch (its version flips 300 times), item 0 in mini-batches 0 and 299 only (first of the first part, last of the second),
    item n_items - 1 in 255 and 256 only (last of the first part, first of the second); every other row at random."""
    B, nb = 4, EVERY_BATCH_BATCHES
    n = B * nb
    special = [0, n_items - 1]
    user = rng.integers(0, n_users - 1, n)
    i = _other_items(rng, n, n_items, np.full(n, -1), exclude=special)
    j = _other_items(rng, n, n_items, i, exclude=special)
    at = np.arange(nb) * B + rng.integers(0, B, nb)
    user[at] = n_users - 1
    for item, batches in ((0, [0, nb - 1]), (n_items - 1, [255, 256])):
        for b in batches:
            i[b * B + int(rng.integers(0, B))] = item
    return _finish(rng, algorithm, user, i, j, B, shuffle=False)


def roles_mixed(n_users, n_items, group, algorithm, rng):
    """BPR, one mini-batch of 17 samples on users 0..15 (sorted positions = the order of the user ids):
      * users 0 .. g-1 once each: an aligned block of `group` lone users (a pair task when g > 1),
      * user g once, user g+1 TWICE: the next block holds a lone user and a run of two, and is broken by it,
      * users g+2 .. 15 once each (whole blocks again, and a last one cut short by the first item),
      * item 0 is the positive item of one sample and the negative item of another; the first of them belongs to a lone user whose
        positive item is therefore shared,
      * item 3 likewise, the other way round,
      * every other item once: a lone user whose two items are touched once is a fully fused sample."""
    assert algorithm == "MF_BPR"
    g = group
    user = np.array(list(range(16)) + [g + 1])
    i = np.concatenate([[0, 2], 3 + np.arange(15)])
    j = np.concatenate([[1, 0], 18 + np.arange(14), [3]])
    return _finish(rng, algorithm, user, i, j, 17)


CASES = {
    "all_threes": all_threes,
    "one_three_rest_single": one_three_rest_single,
    "straddle": straddle,
    "offsets": offsets,
    "one_row_everywhere": one_row_everywhere,
    "partial_tail": partial_tail,
    "partial_tail_one_sample": partial_tail_one_sample,
    "every_batch": every_batch,
    "roles_mixed": roles_mixed,
}
BPR_ONLY = ("roles_mixed",)
# FunkSVD runs these with use_bias: they carry the global-bias ring and Adam's t across mini-batches, calls and schedule parts
FUNK_WITH_BIAS = ("partial_tail", "partial_tail_one_sample", "every_batch")


def cases_of(algorithm):
    return [name for name in CASES if algorithm == "MF_BPR" or name not in BPR_ONLY]


def build(case, n_users, n_items, group, algorithm):
    assert algorithm in ALGORITHMS and group in (1, 2, 4) and (n_users, n_items) in SHAPES
    u, i, third, B = CASES[case](n_users, n_items, group, algorithm, _rng(case, n_users, n_items, group, algorithm))
    assert u.dtype == i.dtype == np.int32 and third.dtype == (np.int32 if algorithm == "MF_BPR" else np.float64)
    assert len(u) == len(i) == len(third) and 0 <= u.min() and u.max() < n_users and 0 <= i.min() and i.max() < n_items
    if algorithm == "MF_BPR":
        assert 0 <= third.min() and third.max() < n_items and (third != i).all()
    else:
        assert set(third.tolist()) <= {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}
    return u, i, third, B
