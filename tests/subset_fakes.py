"""A numpy stand-in for FlatIndex with query_subset, answered by the restatement of tests/subset_cases.py on top of the distinct
stand-in of tests/distinct_fakes.py (so every older call of the host layers is there too, and recorded). Used by
test_subset_layers_cpu.py to exercise the host layers where no GPU exists. Not a test module."""
import numpy as np

import subset_cases as sc
from distinct_fakes import OracleDistinctIndex


class OracleSubsetIndex(OracleDistinctIndex):
    instances = []

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.subset_calls = []           # (Q, k, the list as a tuple, require, exclude) of every subset call
        OracleSubsetIndex.instances.append(self)

    def query_subset(self, queries, k, labels, require=None, exclude=None):
        q = np.asarray(queries, np.float32).reshape(-1, self.dim)
        cand = np.asarray(labels, np.int64).reshape(-1)
        if not 1 <= k <= 2040 or q.shape[0] < 1:
            raise RuntimeError("bad arguments")
        as_int = lambda m: None if m is None else int(np.asarray(m).reshape(-1)[0])   # noqa: E731  (the layers pass one mask for all)
        self.subset_calls.append((q.shape[0], k, tuple(cand.tolist()), as_int(require), as_int(exclude)))
        tags = np.array([self.tags.get(int(l), 0) for l in self.labs], np.uint64)
        return sc.expected_subset(q, k, cand, self.rows, self.labs, tags, require, exclude)

    def other_calls(self):
        """how many calls of any other query kind the index has answered"""
        return self.flat_calls + len(self.probed_calls) + len(self.distinct_calls) + len(self.radius_calls)
