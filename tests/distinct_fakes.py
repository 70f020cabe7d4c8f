"""A numpy stand-in for FlatIndex with query_distinct, answered by the restatement of tests/distinct_cases.py on top of the
partition stand-in of test_partition_layers_cpu.py. Used by test_distinct_layers_cpu.py to exercise the host layers where no GPU
exists. Not a test module."""
import numpy as np

import distinct_cases as dc
from test_partition_layers_cpu import OraclePartitionIndex


class OracleDistinctIndex(OraclePartitionIndex):
    instances = []

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.distinct_calls = []         # (Q, k, min_sep, pool, nprobe, masked) of every distinct call
        OracleDistinctIndex.instances.append(self)

    def query_distinct(self, queries, k, min_sep, pool=None, nprobe=0, require=None, exclude=None):
        from mmiss_amd.index import default_distinct_pool

        q = np.asarray(queries, np.float32).reshape(-1, self.dim)
        pool = default_distinct_pool(k) if pool is None else int(pool)
        if not 1 <= k <= pool <= dc.MAX_POOL or min_sep != min_sep or nprobe < 0:
            raise RuntimeError("bad arguments")
        self.distinct_calls.append((q.shape[0], k, float(min_sep), pool, nprobe, require is not None or exclude is not None))
        part = None
        if nprobe >= 1:
            if self.part is None:
                raise RuntimeError("no partition")
            part = dict(nprobe=nprobe, centres=self.part["centres"], cells=self.part["cells"], B=self.part["B"])
        tags = np.array([self.tags.get(int(l), 0) for l in self.labs], np.uint64)
        return dc.expected_distinct(q, k, pool, min_sep, self.rows, self.labs, tags, require, exclude, partition=part)
