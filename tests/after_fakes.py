"""A numpy stand-in for FlatIndex with query_after, answered by the restatement of tests/after_cases.py on top of the subset
stand-in of tests/subset_fakes.py (so every older call of the host layers is there too, and recorded). Used by
test_after_layers_cpu.py to exercise the host layers where no GPU exists. Not a test module."""
import numpy as np

import after_cases as ac
from subset_fakes import OracleSubsetIndex


class OracleAfterIndex(OracleSubsetIndex):
    instances = []
    MAX_K = 2040                         # (FlatIndex.ranking, borrowed by the tests, reads it)

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.after_calls = []            # (Q, k, cursors as ((distance bits, label), ...), max_dist or None, the list or None, require, exclude)
        OracleAfterIndex.instances.append(self)

    def query_after(self, queries, k, after_dist, after_label, max_dist=None, labels=None, require=None, exclude=None):
        q = np.asarray(queries, np.float32).reshape(-1, self.dim)
        Q = q.shape[0]
        if not 1 <= k <= 2040 or Q < 1:
            raise RuntimeError("bad arguments")
        ad = np.broadcast_to(np.asarray(after_dist, np.float32).reshape(-1), (Q,))
        al = np.broadcast_to(np.asarray(after_label, np.int64).reshape(-1), (Q,))
        as_int = lambda m: None if m is None else int(np.asarray(m).reshape(-1)[0])   # noqa: E731  (the layers pass one mask for all)
        md = None if max_dist is None else float(np.asarray(max_dist, np.float32).reshape(-1)[0])
        cand = None if labels is None else tuple(np.asarray(labels, np.int64).reshape(-1).tolist())
        self.after_calls.append((Q, k, tuple((int(d.view(np.uint32)), int(l)) for d, l in zip(ad, al)), md, cand, as_int(require), as_int(exclude)))
        tags = np.array([self.tags.get(int(l), 0) for l in self.labs], np.uint64)
        return ac.expected_after(q, k, ad, al, self.rows, self.labs, tags, require, exclude, max_dist, None if labels is None else np.asarray(cand, np.int64))

    def other_calls(self):
        """how many calls of any other query kind the index has answered"""
        return super().other_calls() + len(self.subset_calls)
