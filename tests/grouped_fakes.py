"""A numpy stand-in for FlatIndex with set_groups / get_groups / query_grouped, answered by the restatement of
tests/grouped_cases.py on top of the stand-in of after_fakes.py. Used by test_grouped_layers_cpu.py to exercise the host layers
where no GPU exists. Not a test module."""
import numpy as np

import grouped_cases as gc
from after_fakes import OracleAfterIndex


class OracleGroupedIndex(OracleAfterIndex):
    instances = []

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.groups = {}                 # label -> group, as the last set_groups left it (absent: -1)
        self.group_pushes = []           # the labels of every set_groups call, as tuples
        self.grouped_calls = []          # (Q, k, pool, require) of every grouped call
        OracleGroupedIndex.instances.append(self)

    def set_groups(self, labels, groups):
        labels = np.asarray(labels, np.int64).reshape(-1)
        groups = np.asarray(groups).reshape(-1)
        if labels.shape != groups.shape or not np.isin(labels, self.labs).all() or (groups < -1).any() or (groups >= gc.MAX_GROUPS).any():
            raise RuntimeError("bad arguments")
        self.group_pushes.append(tuple(labels.tolist()))
        self.groups.update(zip(labels.tolist(), (int(g) for g in groups)))

    def get_groups(self, labels):
        return np.array([self.groups.get(int(l), -1) for l in np.asarray(labels).reshape(-1)], np.int32)

    def query_grouped(self, queries, k, pool=None, require=None, exclude=None):
        q = np.asarray(queries, np.float32).reshape(-1, self.dim)
        if not 1 <= k <= 2040 or q.shape[0] < 1 or (pool is not None and not k <= pool <= gc.MAX_POOL):
            raise RuntimeError("bad arguments")
        as_int = lambda m: None if m is None else int(np.asarray(m).reshape(-1)[0])   # noqa: E731  (the layers pass one mask for all)
        self.grouped_calls.append((q.shape[0], k, pool, as_int(require)))
        tags = np.array([self.tags.get(int(l), 0) for l in self.labs], np.uint64)
        groups = self.get_groups(self.labs)
        lab, dist, grp, cnt = gc.expected_grouped(q, k, self.rows, self.labs, groups, tags, require, exclude)
        P = gc.default_pool(k) if pool is None else pool
        return lab, dist, grp, cnt, gc.expected_route(q, k, P, self.rows, self.labs, groups, tags, require, exclude)

    def other_calls(self):
        """how many calls of any other query kind the index has answered"""
        return super().other_calls() + len(self.after_calls)
