"""Host paths of csrc/mf.hip that no other GPU test reaches: the group's epoch loop without look-ahead, with per-member schedules and
as plain launches, and a long stream scheduled in one piece instead of FAST_MAX_BATCHES mini-batches at a time.

Every switch is set before the first handle of its case is created and stays as it is while the handles live.
"""
import numpy as np
import pytest

from recsys2019_deeplearning_evaluation_amd import MatrixFactorization_MI355X_Epoch
from recsys2019_deeplearning_evaluation_amd.synthetic import synthetic_urm
from test_mf_gpu import _group_case

pytestmark = pytest.mark.gpu

GROUP_SWITCHES = [None, "MI355REC_MF_GROUP_NO_LOOKAHEAD", "MI355REC_MF_GROUP_PER_MEMBER_SCHEDULE", "MI355REC_NO_GRAPH"]


@pytest.mark.parametrize("switch", GROUP_SWITCHES)
def test_group_paths_end_bit_identical_to_training_alone(gpu, switch, monkeypatch):
    """look-ahead (the second call has two epochs) | one captured graph per epoch | samplers and schedules on the members' own streams |
    plain launches: each member must end exactly where it ends alone, as in test_group_members_end_bit_identical_to_training_alone."""
    if switch:
        monkeypatch.setenv(switch, "1")
    X = synthetic_urm(600, 400, 9000, min_len=2, seed=5)
    assert X.shape[0] // 64 + 1 == 10                       # mini-batches per epoch
    kws = [dict(n_factors=k, algorithm_name="MF_BPR", batch_size=64, random_seed=90 + n, sgd_mode="sgd", learning_rate=0.02 * (n + 1),
                user_reg=0.001 * n, positive_reg=0.002, negative_reg=0.001 * (3 - n)) for n, k in enumerate([8, 12, 16])]
    _group_case(X, kws, epochs=3)                           # two calls: 1 epoch, then 2


def test_whole_stream_schedule_agrees_with_the_schedule_in_parts(gpu, monkeypatch):
    """276 mini-batches: a part of 256 and a short one on the in-LDS schedule, or (MI355REC_MF_WHOLE_STREAM_SCHEDULE) one radix-sort
    schedule of the whole stream.  Same streams; factors as close as test_schedule_paths_agree asks of its two schedules."""
    X = synthetic_urm(1100, 300, 12000, min_len=2, seed=6)
    assert X.shape[0] // 4 + 1 == 276
    kw = dict(n_factors=8, algorithm_name="MF_BPR", batch_size=4, random_seed=12, sgd_mode="sgd", learning_rate=0.02, user_reg=0.01,
              positive_reg=0.01, negative_reg=0.02)
    out = []
    for whole in (False, True):
        if whole:               # (the first pass's handle is closed by now: no handle lives through the change)
            monkeypatch.setenv("MI355REC_MF_WHOLE_STREAM_SCHEDULE", "1")
        dev = MatrixFactorization_MI355X_Epoch(X, **kw)
        dev.epochIteration_Cython(2)
        out.append((dev.get_USER_factors(), dev.get_ITEM_factors(), dev.last_epoch_samples()))
        dev.close()
    assert len(out[0][2][0]) == 276 * 4
    for x, y in zip(out[0][2], out[1][2]):
        np.testing.assert_array_equal(x, y)
    for a, b in zip(out[0][:2], out[1][:2]):
        assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max()
