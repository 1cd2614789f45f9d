"""Phase stamps of the in-LDS schedule's sort kernel at the headline shape (diagnostics; run on the GPU box).
Usage: mf_head_ticks.py [replay]   -- `replay` hands the device's own stream back through replay_samples(): the sort kernel then reads
the stream from memory (the path of a replayed stream, and of every stream before the workgroups drew their own) instead of drawing it."""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["MI355REC_MF_TICKS"] = "1"
from recsys2019_deeplearning_evaluation_amd import MatrixFactorization_MI355X_Epoch, _native as N
from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm
X = named_urm("ml20m", "binary")
m = MatrixFactorization_MI355X_Epoch(X, n_factors=128, algorithm_name="MF_BPR", batch_size=1000, learning_rate=1e-3, sgd_mode="sgd", random_seed=1)
m.epochIteration_Cython(3)
n_batches = X.shape[0] // 1000 + 1
if len(sys.argv) > 1 and sys.argv[1] == "replay":
    u, i, j = m.last_epoch_samples()
    for _ in range(3):
        m.replay_samples(u, i, neg_item=j)
n = C.c_int64(0)
m._call("get_schedule_ticks", None, 0, C.byref(n))
t = np.zeros(n.value, np.uint64)
m._call("get_schedule_ticks", N.ptr(t), n.value, C.byref(n))
t = t.reshape(-1, 8).astype(np.int64)[:n_batches]
names = ("keys in LDS", "radix sort", "run heads", "once-touched flags", "slot scans", "headers + bitmap", "sorted_slot / qtask")
print("%d workgroups; cycles of thread 0 per phase: p50 / p90 / max" % len(t))
for k, name in enumerate(names):
    d = t[:, k + 1] - t[:, k]
    print("%-20s %7d %7d %7d" % (name, np.median(d), np.quantile(d, 0.9), d.max()))
d = t[:, 7] - t[:, 0]
print("%-20s %7d %7d %7d" % ("entry -> exit", np.median(d), np.quantile(d, 0.9), d.max()))
print("first entry -> last exit %d cycles" % (t[:, 7].max() - t[:, 0].min()))
