"""What the step-wise wrappers of PureSVD (pure_svd.py) and NMF (nmf.py) share: a native handle that keeps the URM in both layouts
and one float32 block per side on the device (csrc/blocks.h) -- side 0 is (n_users, width), side 1 is (n_items, width)."""
import ctypes as C

import numpy as np

from . import _native as N


class BlockPairSteps(N.Handle):
    _SIDE_NAMES = None                # the wrapper's words for side 0 and side 1, as its ValueError names them

    def __init__(self, URM_train, width):
        X, arrays = N.both_layouts(URM_train)
        self.n_users, self.n_items = X.shape
        self.width = int(width)
        self.nnz = int(X.nnz)
        self._create(self.n_users, self.n_items, self.width, *[N.ptr(a) for a in arrays])

    def rows_of(self, side):
        return self.n_items if side else self.n_users

    def _side(self, side):
        if side not in (0, 1):
            raise ValueError("side %r: 0 (%s) or 1 (%s)" % ((side,) + tuple(self._SIDE_NAMES)))
        return int(side)

    def set_block(self, side, X):
        X = N.as_f32(X)
        if X.shape != (self.rows_of(self._side(side)), self.width):
            raise ValueError("block of side %r must be %d x %d, got %r" % (side, self.rows_of(side), self.width, X.shape))
        self._call("set_block", side, N.ptr(X))

    def get_block(self, side):
        X = np.empty((self.rows_of(self._side(side)), self.width), np.float32)
        self._call("get_block", side, N.ptr(X))
        return X

    def _fit_info_tail(self, *phase_args):
        """Calls fit_info with the wrapper's own phase arguments in front; returns the part both handles report: the traffic counters."""
        v = [C.c_int64() for _ in range(5)]
        ones = C.c_int32()
        self._call("fit_info", *phase_args, *[C.byref(x) for x in v], C.byref(ones))
        return {"launches": v[0].value, "calls": v[1].value, "create_bytes": v[2].value, "h2d_bytes": v[3].value, "d2h_bytes": v[4].value,
                "all_ones": bool(ones.value)}
