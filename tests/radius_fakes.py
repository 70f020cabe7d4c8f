"""A numpy stand-in for FlatIndex with its radius queries (and the tag words they combine with), answered by the oracle through
tests/radius_cases.py. Used by test_radius_layers_cpu.py to exercise the host layers where no GPU exists. Not a test module."""
import numpy as np

import radius_cases as rc
from fakes import OracleIndex
from oracle import retrieval_oracle as ro


class OracleRadiusIndex(OracleIndex):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.tags = {}
        self.radius_calls = []       # (kind, radius, cap) of every radius call

    def set_tags(self, labels, tags):
        self.tags.update(zip((int(x) for x in np.asarray(labels).reshape(-1)), (int(x) for x in np.asarray(tags, np.uint64).reshape(-1))))

    def _admit(self, Q, require, exclude):
        req = np.broadcast_to(np.asarray(0 if require is None else require, np.uint64), (Q,))
        exc = np.broadcast_to(np.asarray(0 if exclude is None else exclude, np.uint64), (Q,))
        tags = np.array([self.tags.get(int(l), 0) for l in self.labs], np.uint64)
        return lambda j: ((tags & req[j]) == req[j]) & ((tags & exc[j]) == 0)

    def query(self, q, k, require=None, exclude=None):
        if require is None and exclude is None:
            return super().query(q, k)
        q = np.asarray(q, np.float32).reshape(-1, self.dim)
        admit = self._admit(q.shape[0], require, exclude)
        out = [np.full((q.shape[0], k), -1, np.int64), np.full((q.shape[0], k), np.inf, np.float32), np.zeros(q.shape[0], np.int32)]
        for i in range(q.shape[0]):
            sub = np.nonzero(admit(i))[0]
            if sub.size:
                ol, od, oc = ro.query(q[i:i + 1], self.rows[sub], self.labs[sub], k)
                out[0][i], out[1][i], out[2][i] = ol[0], od[0], oc[0]
        return tuple(out)

    def query_radius(self, queries, max_dist, cap=1000, require=None, exclude=None):
        q = np.asarray(queries, np.float32).reshape(-1, self.dim)
        if np.isnan(np.asarray(max_dist, np.float32)).any():
            raise RuntimeError("max_dist is NaN")
        self.radius_calls.append(("query", max_dist, cap))
        if self.labs.size == 0:
            return (np.full((q.shape[0], cap), -1, np.int64), np.full((q.shape[0], cap), np.inf, np.float32),
                    np.zeros(q.shape[0], np.int32), np.zeros(q.shape[0], np.int64))
        masked = require is not None or exclude is not None
        return rc.expected(q, self.rows, self.labs, max_dist, cap, admit=self._admit(q.shape[0], require, exclude) if masked else None)

    def query_radius_by_label(self, labels, max_dist, cap, later_only=False):
        labels = np.asarray(labels, np.int64).reshape(-1)
        rows = np.searchsorted(self.labs, labels)
        if (rows >= self.labs.size).any() or (self.labs[np.minimum(rows, self.labs.size - 1)] != labels).any():
            raise RuntimeError("label not in the index")
        self.radius_calls.append(("by_label", max_dist, cap))
        return rc.expected(rc.represented(self.rows)[rows], self.rows, self.labs, max_dist, cap, row_min=rows if later_only else None)

    def near_duplicates(self, max_dist, cap_per_row=64):
        from mmiss_amd.index import FlatIndex

        return FlatIndex.near_duplicates(self, max_dist, cap_per_row)     # (the product's own walk, over this index's calls)
