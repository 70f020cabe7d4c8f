"""FlatIndex — one shard of the in-HBM flat cosine index (libmmiss `mmiss_index_*`).

Numeric half of the chromadb Collection the reference creates with {"hnsw:space": "cosine"}
(backend/app/utils.py:127-130): rows are L2-normalised when added; a query returns the k rows of
smallest cosine distance 1 - cos, ascending, ties by label ascending.
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Optional, Tuple

import numpy as np

from . import _lib

F32, F16, F8 = _lib.MMISS_F32, _lib.MMISS_F16, _lib.MMISS_F8
_DTYPES = {"f32": F32, "float32": F32, "f16": F16, "float16": F16, "f8": F8, "fp8": F8, "e4m3": F8, F32: F32, F16: F16, F8: F8}


MAX_POOL = 2040   # mmiss_index_query_distinct's limit on pool (the list calls' own limit on k)
MAX_GROUPS = 1 << 24   # MMISS_MAX_GROUPS: group ids are -1 (none) .. MAX_GROUPS - 1


def _is_torch(x) -> bool:
    return hasattr(x, "data_ptr")


def default_distinct_pool(k: int) -> int:
    """the list length FlatIndex.query_distinct walks when the caller names none"""
    return min(MAX_POOL, max(8 * int(k), 64))


class FlatIndex:
    def __init__(self, dim: int, dtype="f32", device: int = 0, capacity: int = 0):
        self.dim = int(dim)
        self.dtype = _DTYPES[dtype]
        self.device = int(device)
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self._lib.mmiss_index_create(self.dim, self.dtype, self.device, int(capacity), C.byref(h)))
        self._h = h
        # re-entrant: a PendingQuery collected by the cyclic GC on a thread that is inside one of these calls must not
        # deadlock that thread on itself
        self._call_lock = threading.RLock()
        # generation of the handle's ONE open-query slot: bumped by every query_begin, result and abort. A PendingQuery only
        # ends / aborts the C-side query while its own generation is still the current one, so a stale handle that outlives
        # its query (kept alive by a traceback or a reference cycle) cannot abort a newer query of someone else.
        self._query_gen = 0

    # ------------------------------------------------------------------ helpers
    def _vecs(self, v):
        if _is_torch(v):
            import torch

            v = v.to(torch.float32).contiguous()
        else:
            v = np.ascontiguousarray(v, dtype=np.float32)
        if v.ndim == 1:
            v = v.reshape(1, -1)
        if v.ndim != 2 or v.shape[1] != self.dim:
            raise ValueError(f"expected [n,{self.dim}] vectors, got {tuple(v.shape)}")
        return v

    def _sync_stream(self, x):
        if _is_torch(x) and x.is_cuda:
            _lib.check(self._lib.mmiss_index_set_stream(self._h, _lib.current_stream_ptr(x.device), 0))
        else:
            _lib.check(self._lib.mmiss_index_set_stream(self._h, None, 1))

    # ------------------------------------------------------------------ mutation
    def add(self, vecs, labels) -> None:
        v = self._vecs(vecs)
        lab = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
        if lab.shape[0] != v.shape[0]:
            raise ValueError("labels and vectors differ in length")
        with self._call_lock:  # stream hand-over + call are one unit per handle (threads: pipeline.BatchLanes)
            self._sync_stream(v)
            _lib.check(self._lib.mmiss_index_add(self._h, _lib.ptr(v), lab.ctypes.data, int(v.shape[0])))

    def update(self, labels, vecs) -> None:
        v = self._vecs(vecs)
        lab = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
        with self._call_lock:  # stream hand-over + call are one unit per handle (threads: pipeline.BatchLanes)
            self._sync_stream(v)
            _lib.check(self._lib.mmiss_index_update(self._h, lab.ctypes.data, _lib.ptr(v), int(v.shape[0])))

    def remove(self, labels) -> int:
        lab = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
        n = C.c_int64(0)
        _lib.check(self._lib.mmiss_index_remove(self._h, lab.ctypes.data, int(lab.shape[0]), C.byref(n)))
        return n.value

    def clear(self) -> None:
        _lib.check(self._lib.mmiss_index_clear(self._h))

    # ------------------------------------------------------------------ read
    def count(self) -> int:
        n = C.c_int64(0)
        _lib.check(self._lib.mmiss_index_count(self._h, C.byref(n)))
        return n.value

    def __len__(self) -> int:
        return self.count()

    def labels(self) -> np.ndarray:
        n = self.count()
        out = np.empty(n, dtype=np.int64)
        _lib.check(self._lib.mmiss_index_labels(self._h, out.ctypes.data, n))
        return out

    def get(self, labels) -> np.ndarray:
        lab = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
        out = np.empty((lab.shape[0], self.dim), dtype=np.float32)
        if lab.shape[0]:
            _lib.check(self._lib.mmiss_index_get(self._h, lab.ctypes.data, int(lab.shape[0]), out.ctypes.data))
        return out

    # ------------------------------------------------------------------ tags (filtered queries)
    def set_tags(self, labels, tags) -> None:
        """Per-row 64-bit tag words (mmiss_index_set_tags): labels [n], tags [n] (uint64, or int64 bit patterns). A label not in
        the index raises and changes nothing. Rows are added with tag 0; update keeps a row's tag; load resets every tag to 0."""
        lab = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
        t = np.asarray(tags)
        if t.dtype.kind not in "ui" and not (t.dtype == object and t.size == 0):
            raise TypeError(f"tags must be integers, got {t.dtype}")
        t = np.ascontiguousarray(t.astype(np.int64, copy=False).view(np.uint64) if t.dtype.kind == "i" else t.astype(np.uint64)).reshape(-1)
        if t.shape[0] != lab.shape[0]:
            raise ValueError(f"{lab.shape[0]} labels but {t.shape[0]} tags")
        with self._call_lock:
            _lib.check(self._lib.mmiss_index_set_tags(self._h, lab.ctypes.data, t.ctypes.data, int(lab.shape[0])))

    def get_tags(self, labels) -> np.ndarray:
        """-> uint64 [n], the tag words of `labels` (a label not in the index raises)."""
        lab = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
        out = np.zeros(lab.shape[0], dtype=np.uint64)
        if lab.shape[0]:
            with self._call_lock:
                _lib.check(self._lib.mmiss_index_get_tags(self._h, lab.ctypes.data, int(lab.shape[0]), out.ctypes.data))
        return out

    @staticmethod
    def _mask(m, Q: int, q, name: str):
        """A query mask -> None, a uint64 numpy [Q], or a contiguous int64 CUDA tensor [Q] (bit patterns). A scalar is the same
        mask for every query. CUDA masks go with CUDA queries (they are read on the query's stream)."""
        if m is None:
            return None
        if _is_torch(m):
            import torch

            if m.dtype.is_floating_point or m.dtype == torch.bool or m.dtype.is_complex:
                raise TypeError(f"{name}: integer mask expected, got {m.dtype}")
            if m.dim() == 0:
                m = m.reshape(1).expand(Q)
            if m.dim() != 1 or int(m.shape[0]) != Q:
                raise ValueError(f"{name}: expected a scalar or [{Q}] masks, got shape {tuple(m.shape)}")
            if m.is_cuda:
                if m.dtype != torch.int64 and str(m.dtype) != "torch.uint64":
                    m = m.to(torch.int64)
                return m.contiguous()
            m = m.cpu().numpy()
        if isinstance(m, (bool, np.bool_)) or isinstance(m, float) or isinstance(m, np.floating):
            raise TypeError(f"{name}: integer mask expected, got {type(m).__name__}")
        if isinstance(m, (int, np.integer)):
            v = int(m)
            if not -(1 << 63) <= v < (1 << 64):
                raise ValueError(f"{name}: {v} does not fit 64 bits")
            return np.full(Q, v & ((1 << 64) - 1), dtype=np.uint64)
        a = np.asarray(m)
        if a.dtype.kind not in "ui":
            raise TypeError(f"{name}: integer mask expected, got {a.dtype}")
        if a.ndim == 0:
            a = np.full(Q, a, dtype=a.dtype)
        if a.ndim != 1 or a.shape[0] != Q:
            raise ValueError(f"{name}: expected a scalar or [{Q}] masks, got shape {a.shape}")
        a = a.astype(np.int64, copy=False).view(np.uint64) if a.dtype.kind == "i" else a.astype(np.uint64, copy=False)
        return np.ascontiguousarray(a)

    def query(self, queries, k: int, require=None, exclude=None) -> Tuple["np.ndarray", "np.ndarray", "np.ndarray"]:
        """-> (labels int64 [Q,k], distances float32 [Q,k], counts int32 [Q]); numpy in -> numpy out,
        CUDA tensor in -> CUDA tensors out (no host round trip).
        require / exclude (filtered query, mmiss_index_query_filtered): row r is admitted for query q iff
        (tags[r] & require[q]) == require[q] and (tags[r] & exclude[q]) == 0, and the result is the exact top-k among admitted
        rows. Each is a scalar (every query) or [Q] integers, numpy or a CUDA tensor; None = 0. Both None: mmiss_index_query."""
        return self._query(queries, k, split=False, require=require, exclude=exclude)

    def query_begin(self, queries, k: int, require=None, exclude=None) -> "PendingQuery":
        """Queue the query's first pass and return at once (mmiss_index_query_begin); `.result()` of the returned handle waits
        for it, widens what the exactness guard could not prove, and returns what query() returns. Between the two the caller
        may queue other GPU work on the same stream (the next batch's encode) — but no other call on this index.
        require / exclude as in query()."""
        return self._query(queries, k, split=True, require=require, exclude=exclude)

    def query_next(self, pending: "PendingQuery", queries, k: int, require=None, exclude=None):
        """`pending.result()` and `query_begin(queries, k)` back to back -> (results of `pending`, the new PendingQuery). Everything
        Python has to do for the NEW query (layout checks, output buffers) happens BEFORE the pending one is ended, so between the
        last operation of its widen pass and the first kernel of the new first pass lie two C calls and nothing else. In a serving
        loop that keeps one query batch open per step (bench.py) the GPU idled ~87 us per step there (rocprofv3 kernel trace of
        round 6: the gap between the widen pass's count readback and prep_queries_kernel). Since the library runs the widen pass
        on the handle's side stream, the 39 us that were left of it no longer idle the GPU either: the next batch's encode,
        already queued on the caller's stream, runs through them (6 us in front of prep_queries_kernel in the same kind of trace)."""
        q, outs = self._prepare(queries, k)
        masks = self._masks(q, require, exclude)
        prev = pending.result()
        with self._call_lock:
            self._sync_stream(q)
            if masks is None:
                _lib.check(self._lib.mmiss_index_query_begin(self._h, _lib.ptr(q), int(q.shape[0]), int(k), _lib.ptr(outs[0]), _lib.ptr(outs[1]),
                                                             _lib.ptr(outs[2])))
            else:
                _lib.check(self._lib.mmiss_index_query_filtered_begin(self._h, _lib.ptr(q), int(q.shape[0]), int(k), _lib.ptr(masks[0]),
                                                                      _lib.ptr(masks[1]), _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2])))
            self._query_gen += 1
            return prev, PendingQuery(self, q, outs, self._query_gen, masks)

    def _masks(self, q, require, exclude):
        """(require, exclude) in the form the C call takes, or None when both are None (the unfiltered call)."""
        if require is None and exclude is None:
            return None
        Q = int(q.shape[0])
        return (self._mask(require, Q, q, "require"), self._mask(exclude, Q, q, "exclude"))

    def _prepare(self, queries, k: int):
        q = self._vecs(queries)
        Q = int(q.shape[0])
        if _is_torch(q) and q.is_cuda:
            import torch

            lab = torch.empty((Q, k), dtype=torch.int64, device=q.device)
            dist = torch.empty((Q, k), dtype=torch.float32, device=q.device)
            cnt = torch.empty((Q,), dtype=torch.int32, device=q.device)
        else:
            if _is_torch(q):
                q = q.numpy()
            lab = np.empty((Q, k), dtype=np.int64)
            dist = np.empty((Q, k), dtype=np.float32)
            cnt = np.empty((Q,), dtype=np.int32)
        return q, (lab, dist, cnt)

    def _query(self, queries, k: int, split: bool, require=None, exclude=None):
        q, (lab, dist, cnt) = self._prepare(queries, k)
        Q = int(q.shape[0])
        masks = self._masks(q, require, exclude)
        with self._call_lock:  # stream hand-over + call are one unit per handle (threads: pipeline.BatchLanes)
            self._sync_stream(q)
            if masks is None:
                fn = self._lib.mmiss_index_query_begin if split else self._lib.mmiss_index_query
                _lib.check(fn(self._h, _lib.ptr(q), Q, int(k), _lib.ptr(lab), _lib.ptr(dist), _lib.ptr(cnt)))
            else:
                fn = self._lib.mmiss_index_query_filtered_begin if split else self._lib.mmiss_index_query_filtered
                _lib.check(fn(self._h, _lib.ptr(q), Q, int(k), _lib.ptr(masks[0]), _lib.ptr(masks[1]), _lib.ptr(lab), _lib.ptr(dist),
                              _lib.ptr(cnt)))
            if split:
                self._query_gen += 1
                return PendingQuery(self, q, (lab, dist, cnt), self._query_gen, masks)
        return (lab, dist, cnt)

    # ------------------------------------------------------------------ radius queries
    def _radius_outputs(self, Q: int, cap: int, like=None):
        if like is not None:
            import torch

            dev = like.device
            return (torch.empty((Q, cap), dtype=torch.int64, device=dev), torch.empty((Q, cap), dtype=torch.float32, device=dev),
                    torch.empty((Q,), dtype=torch.int32, device=dev), torch.empty((Q,), dtype=torch.int64, device=dev))
        # (filled here: a call of no queries writes nothing)
        return (np.full((Q, cap), -1, dtype=np.int64), np.full((Q, cap), np.inf, dtype=np.float32),
                np.zeros((Q,), dtype=np.int32), np.zeros((Q,), dtype=np.int64))

    def query_radius(self, queries, max_dist, cap: int = 1000, require=None, exclude=None):
        """Every row within cosine distance max_dist of each query, exactly (mmiss_index_query_radius) -> (labels int64 [Q, cap],
        distances float32 [Q, cap], counts int32 [Q], totals int64 [Q]): row r is a member of query q iff it has a direction, q
        admits it (require / exclude as in query()) and its distance — the bits query() returns — is <= max_dist[q] as floats.
        totals = the members there are, counts = min(cap, totals), the slots the counts nearest members by (distance, label),
        unused ones -1 / +inf. max_dist: a scalar (every query) or [Q], numpy or a CUDA tensor; NaN raises. cap: 1 .. 4096.
        numpy in -> numpy out, CUDA tensor in -> CUDA tensors out."""
        q = self._vecs(queries)
        Q = int(q.shape[0])
        cuda = _is_torch(q) and q.is_cuda
        if _is_torch(q) and not cuda:
            q = q.numpy()
        if _is_torch(max_dist) and max_dist.is_cuda and cuda:
            import torch

            r = max_dist.to(torch.float32)
            r = (r.reshape(1).expand(Q) if r.dim() == 0 else r).contiguous()
        else:
            if _is_torch(max_dist):
                max_dist = max_dist.detach().cpu().numpy()
            r = np.asarray(max_dist, dtype=np.float32)
            r = np.ascontiguousarray(np.full(Q, r, dtype=np.float32) if r.ndim == 0 else r)
        if r.ndim != 1 or int(r.shape[0]) != Q:
            raise ValueError(f"max_dist: expected a scalar or [{Q}] radii, got shape {tuple(r.shape)}")
        masks = self._masks(q, require, exclude) or (None, None)
        lab, dist, cnt, tot = self._radius_outputs(Q, int(cap), q if cuda else None)
        with self._call_lock:
            self._sync_stream(q)
            _lib.check(self._lib.mmiss_index_query_radius(self._h, _lib.ptr(q), Q, _lib.ptr(r), int(cap), _lib.ptr(masks[0]),
                                                          _lib.ptr(masks[1]), _lib.ptr(lab), _lib.ptr(dist), _lib.ptr(cnt), _lib.ptr(tot)))
        return lab, dist, cnt, tot

    def query_radius_by_label(self, labels, max_dist: float, cap: int, later_only: bool = False, device=None):
        """query_radius with the rows the index represents under `labels` as the queries (mmiss_index_query_radius_by_label):
        exactly query_radius(self.get(labels), max_dist, cap), without the rows leaving the device. later_only: only rows whose
        label is greater than the query's own are admitted (no self match; every pair once, the smaller label as the query). A
        label that is not stored raises and writes nothing. device: a torch device for CUDA outputs; numpy outputs otherwise."""
        lab_in = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
        n = int(lab_in.shape[0])
        like = None
        if device is not None:
            import torch

            like = torch.empty(0, device=device)
        lab, dist, cnt, tot = self._radius_outputs(n, int(cap), like)
        with self._call_lock:
            self._sync_stream(like)
            _lib.check(self._lib.mmiss_index_query_radius_by_label(self._h, lab_in.ctypes.data, n, float(max_dist), int(cap),
                                                                   1 if later_only else 0, _lib.ptr(lab), _lib.ptr(dist), _lib.ptr(cnt),
                                                                   _lib.ptr(tot)))
        return lab, dist, cnt, tot

    def near_duplicates(self, max_dist: float, cap_per_row: int = 64):
        """Every pair of stored rows within cosine distance max_dist, each once -> (a int64 [P], b int64 [P], dist float32 [P],
        overflow): labels a < b, ordered by (a, dist, b); overflow = {label: total} for the rows with more than cap_per_row
        later partners (of those the cap_per_row nearest are reported). Walks the labels in chunks of 1024 through
        query_radius_by_label(later_only=True)."""
        labels = self.labels()
        pa, pb, pd, overflow = [], [], [], {}
        for i0 in range(0, labels.shape[0], 1024):
            chunk = labels[i0:i0 + 1024]
            lab, dist, cnt, tot = self.query_radius_by_label(chunk, max_dist, cap_per_row, later_only=True)
            keep = np.arange(lab.shape[1])[None, :] < cnt[:, None]
            pa.append(np.repeat(chunk, cnt))
            pb.append(lab[keep])
            pd.append(dist[keep])
            for j in np.nonzero(tot > cap_per_row)[0]:
                overflow[int(chunk[j])] = int(tot[j])
        if not pa:
            return np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0, np.float32), overflow
        return np.concatenate(pa), np.concatenate(pb), np.concatenate(pd), overflow

    # ------------------------------------------------------------------ membership / tagging
    def _probes(self, queries, max_dist):
        """(queries [P, dim], radii [P], cuda) in the form the membership calls take: numpy arrays, or CUDA tensors for CUDA
        queries. max_dist: a scalar (every probe) or [P], as in query_radius."""
        q = self._vecs(queries)
        P = int(q.shape[0])
        cuda = _is_torch(q) and q.is_cuda
        if _is_torch(q) and not cuda:
            q = q.numpy()
        if _is_torch(max_dist) and max_dist.is_cuda and cuda:
            import torch

            r = max_dist.to(torch.float32)
            r = (r.reshape(1).expand(P) if r.dim() == 0 else r).contiguous()
        else:
            if _is_torch(max_dist):
                max_dist = max_dist.detach().cpu().numpy()
            r = np.asarray(max_dist, dtype=np.float32)
            r = np.ascontiguousarray(np.full(P, r, dtype=np.float32) if r.ndim == 0 else r)
        if r.ndim != 1 or int(r.shape[0]) != P:
            raise ValueError(f"max_dist: expected a scalar or [{P}] radii, got shape {tuple(r.shape)}")
        return q, r, cuda

    def membership(self, queries, max_dist):
        """The exact membership of EVERY row in up to 64 radii, one pass (mmiss_index_membership) -> (words, members): bit p of
        words[r] = row r (the order of labels()) lies within cosine distance max_dist[p] of queries[p] — the member definition of
        query_radius, with no cap on the members —, bits >= P zero; members[p] = how many rows. queries [P, dim], 1 <= P <= 64;
        max_dist a scalar or [P]; NaN raises. numpy in -> uint64 [count] and int64 [P]; CUDA tensors in -> a CUDA int64 tensor of
        the same bit patterns and a CUDA int64 tensor."""
        q, r, cuda = self._probes(queries, max_dist)
        P = int(q.shape[0])
        with self._call_lock:
            n = self.count()
            if cuda:
                import torch

                words = torch.zeros((n,), dtype=torch.int64, device=q.device)
                members = torch.zeros((P,), dtype=torch.int64, device=q.device)
            else:
                words = np.zeros(n, dtype=np.uint64)
                members = np.zeros(P, dtype=np.int64)
            self._sync_stream(q)
            _lib.check(self._lib.mmiss_index_membership(self._h, _lib.ptr(q), P, _lib.ptr(r), _lib.ptr(words), n, _lib.ptr(members)))
        return words, members

    def tag_by_radius(self, queries, max_dist, bits):
        """membership() written straight into the rows' tag words (mmiss_index_tag_by_radius): bit bits[p] of every row's tag
        becomes "row is a member of probe p" (set or cleared), every other bit keeps its value -> members (int64 [P], numpy or
        CUDA as the queries). bits: [P] distinct integers in 0 .. 63."""
        q, r, cuda = self._probes(queries, max_dist)
        P = int(q.shape[0])
        b = np.asarray(bits)
        if b.dtype.kind not in "ui" or isinstance(bits, (bool, np.bool_)):
            raise TypeError(f"bits must be integers, got {b.dtype}")
        b = np.ascontiguousarray(b.reshape(-1).astype(np.int64))
        if b.shape[0] != P:
            raise ValueError(f"{P} probes but {b.shape[0]} bits")
        b = np.ascontiguousarray(np.clip(b, -1, 64).astype(np.int32))   # (out of range stays out of range: the call refuses it)
        if cuda:
            import torch

            members = torch.zeros((P,), dtype=torch.int64, device=q.device)
        else:
            members = np.zeros(P, dtype=np.int64)
        with self._call_lock:
            self._sync_stream(q)
            _lib.check(self._lib.mmiss_index_tag_by_radius(self._h, _lib.ptr(q), P, _lib.ptr(r), b.ctypes.data, _lib.ptr(members)))
        return members

    # ------------------------------------------------------------------ assignment / clustering
    MAX_CENTRES = 1024

    def _centres(self, centres):
        """(centres [C, dim], cuda) in the form the assign call takes; C outside 1 .. MAX_CENTRES raises"""
        c = self._vecs(centres)
        cuda = _is_torch(c) and c.is_cuda
        if _is_torch(c) and not cuda:
            c = c.numpy()
        if not 1 <= int(c.shape[0]) <= self.MAX_CENTRES:
            raise ValueError(f"centres: 1 .. {self.MAX_CENTRES} vectors per call, got {int(c.shape[0])}")
        return c, cuda

    def assign(self, centres, want_dist: bool = True):
        """For EVERY row, the nearest of the C centres (mmiss_index_assign) -> (assign, dist | None, sizes): assign[r] (int32, the
        order of labels()) = the centre of smallest cosine distance to row r — exactly: the c that minimises (d(centre c, row r), c)
        with d the distance query() reports, so ties go to the smaller index —, dist[r] that distance (float32; None unless
        want_dist), sizes[c] (int64) the rows assigned to c. A row without a direction gets -1 / +inf, a centre without one is
        never chosen. centres [C, dim], 1 <= C <= 1024, any norm. numpy in -> numpy out, CUDA tensors in -> CUDA tensors out."""
        c, cuda = self._centres(centres)
        Cn = int(c.shape[0])
        with self._call_lock:
            n = self.count()
            if cuda:
                import torch

                asg = torch.full((n,), -1, dtype=torch.int32, device=c.device)
                dist = torch.full((n,), float("inf"), dtype=torch.float32, device=c.device) if want_dist else None
                sizes = torch.zeros((Cn,), dtype=torch.int64, device=c.device)
            else:
                asg = np.full(n, -1, dtype=np.int32)
                dist = np.full(n, np.inf, dtype=np.float32) if want_dist else None
                sizes = np.zeros(Cn, dtype=np.int64)
            self._sync_stream(c)
            _lib.check(self._lib.mmiss_index_assign(self._h, _lib.ptr(c), Cn, _lib.ptr(asg), _lib.ptr(dist) if want_dist else None, n,
                                                    _lib.ptr(sizes)))
        return asg, dist, sizes

    def cluster_sums(self, assign, n_clusters: int):
        """Per cluster, the sum of its rows in 2^-32 fixed point (mmiss_index_cluster_sums) -> (sums int64 [C, dim], sizes int64
        [C]): sums[c][j] = the sum over the rows r with assign[r] == c of rint(float64(x[r][j]) * 2^32), x = what get() returns —
        one value whatever order the GPU adds in. assign: int32 [count] (numpy or a CUDA tensor; entries outside 0 .. C-1 are
        skipped). numpy in -> numpy out, CUDA in -> CUDA out."""
        Cn = int(n_clusters)
        if not 1 <= Cn <= self.MAX_CENTRES:
            raise ValueError(f"n_clusters: 1 .. {self.MAX_CENTRES}, got {Cn}")
        cuda = _is_torch(assign) and assign.is_cuda
        if cuda:
            import torch

            if assign.dtype.is_floating_point or assign.dtype == torch.bool:
                raise TypeError(f"assign must be integers, got {assign.dtype}")
            a = assign.to(torch.int32).contiguous()
        else:
            a = np.asarray(assign.numpy() if _is_torch(assign) else assign)
            if a.dtype.kind not in "ui":
                raise TypeError(f"assign must be integers, got {a.dtype}")
            a = np.ascontiguousarray(a.astype(np.int32))
        if a.ndim != 1:
            raise ValueError(f"assign: expected one entry per row, got shape {tuple(a.shape)}")
        with self._call_lock:
            n = self.count()
            if int(a.shape[0]) != n:
                raise ValueError(f"assign: {int(a.shape[0])} entries for {n} rows")
            if cuda:
                sums = torch.zeros((Cn, self.dim), dtype=torch.int64, device=a.device)
                sizes = torch.zeros((Cn,), dtype=torch.int64, device=a.device)
            else:
                sums = np.zeros((Cn, self.dim), dtype=np.int64)
                sizes = np.zeros(Cn, dtype=np.int64)
            self._sync_stream(a)
            _lib.check(self._lib.mmiss_index_cluster_sums(self._h, _lib.ptr(a), n, Cn, _lib.ptr(sums), _lib.ptr(sizes)))
        return sums, sizes

    def kmeans(self, n_clusters: int, iters: int = 10, init=None) -> dict:
        """Spherical k-means over the stored rows, deterministic by construction -> dict(centres float32 [C, dim], assign int32
        [count], dist float32 [count], sizes int64 [C], iterations).
        Initial centres: get() of the rows under `init` (labels, length C); None: the rows at positions floor(i * count / C).
        Up to `iters` times: assign (no distances); stop when the assignment equals the previous one; otherwise
        centres[c] = float32(float64(sums[c]) * 2^-32) from cluster_sums — a cluster that is empty, or whose sum is all zero,
        keeps its centre; no re-normalisation, assign() normalises. `iterations` counts the centre updates. One more assign with
        distances follows the loop: the returned assignment always belongs to the returned centres."""
        Cn, iters = int(n_clusters), int(iters)
        if not 1 <= Cn <= self.MAX_CENTRES:
            raise ValueError(f"n_clusters: 1 .. {self.MAX_CENTRES}, got {Cn}")
        if iters < 0:
            raise ValueError(f"iters: {iters}")
        with self._call_lock:
            labels = self.labels()
            n = int(labels.shape[0])
            if init is None:
                if n < 1:
                    raise ValueError("kmeans on an empty index")
                init = labels[(np.arange(Cn, dtype=np.int64) * n) // Cn]
            init = np.ascontiguousarray(init, dtype=np.int64).reshape(-1)
            if init.shape[0] != Cn:
                raise ValueError(f"init: {init.shape[0]} labels for {Cn} clusters")
            centres = np.ascontiguousarray(self.get(init), dtype=np.float32)
            prev, done = None, 0
            for _ in range(iters):
                asg, _d, _s = self.assign(centres, want_dist=False)
                if prev is not None and np.array_equal(asg, prev):
                    break
                prev = asg
                sums, sizes = self.cluster_sums(asg, Cn)
                new = (sums.astype(np.float64) * 2.0 ** -32).astype(np.float32)
                keep = (sizes == 0) | ~sums.any(axis=1)
                new[keep] = centres[keep]
                centres = new
                done += 1
            asg, dist, sizes = self.assign(centres, want_dist=True)
        return {"centres": centres, "assign": asg, "dist": dist, "sizes": sizes, "iterations": done}

    # ------------------------------------------------------------------ partitioned search
    MAX_K = 2040
    PARTITION_INFO_FIELDS = ("cells", "rows", "tail", "rows_in_cells", "largest_cell", "empty_cells", "queries", "scanned")

    def set_partition(self, centres, cells) -> None:
        """Give the index a partition (mmiss_index_partition_set): centres [C, dim] (1 <= C <= 1024, any norm) and cells int32
        [count], the cell of every row in the order of labels() (an entry outside 0 .. C-1, assign()'s -1, puts the row in no
        cell) — what assign() / kmeans() return. numpy arrays or CUDA tensors, each. Rows added later are the tail: candidates
        of every probed query. update / remove / clear / load drop the partition; save does not persist it."""
        c, _cuda = self._centres(centres)
        cuda_cells = _is_torch(cells) and cells.is_cuda
        if cuda_cells:
            import torch

            if cells.dtype.is_floating_point or cells.dtype == torch.bool:
                raise TypeError(f"cells must be integers, got {cells.dtype}")
            a = cells.to(torch.int32).contiguous()
        else:
            a = np.asarray(cells.numpy() if _is_torch(cells) else cells)
            if a.dtype.kind not in "ui":
                raise TypeError(f"cells must be integers, got {a.dtype}")
            a = np.ascontiguousarray(a.astype(np.int32))
        if a.ndim != 1:
            raise ValueError(f"cells: expected one entry per row, got shape {tuple(a.shape)}")
        with self._call_lock:
            self._sync_stream(c if _cuda else (a if cuda_cells else None))
            _lib.check(self._lib.mmiss_index_partition_set(self._h, _lib.ptr(c), int(c.shape[0]), _lib.ptr(a) if a.shape[0] else None,
                                                           int(a.shape[0])))

    def clear_partition(self) -> None:
        with self._call_lock:
            _lib.check(self._lib.mmiss_index_partition_clear(self._h))

    def partition_info(self) -> dict:
        """mmiss_index_partition_info as a dict: cells (C; 0 = no partition), rows (B, the rows it was set on), tail (rows added
        since), rows_in_cells, largest_cell, empty_cells, queries (probed queries served since it was set), scanned (rows they
        looked at)."""
        out = (C.c_int64 * 8)()
        with self._call_lock:
            _lib.check(self._lib.mmiss_index_partition_info(self._h, out))
        return dict(zip(self.PARTITION_INFO_FIELDS, (int(v) for v in out)))

    def partition(self):
        """The partition as stored (mmiss_index_partition_get) -> (centres float32 [C, dim], NORMALISED; cells int32 [B]; sizes
        int64 [C]), numpy. No partition raises."""
        with self._call_lock:
            info = self.partition_info()
            if info["cells"] == 0:
                _lib.check(self._lib.mmiss_index_partition_get(self._h, None, None, 0, None))   # (raises: no partition)
            centres = np.empty((info["cells"], self.dim), dtype=np.float32)
            cells = np.empty(info["rows"], dtype=np.int32)
            sizes = np.empty(info["cells"], dtype=np.int64)
            _lib.check(self._lib.mmiss_index_partition_get(self._h, centres.ctypes.data, cells.ctypes.data if cells.size else None,
                                                           int(cells.shape[0]), sizes.ctypes.data))
        return centres, cells, sizes

    def build_partition(self, n_cells: int, iters: int = 10, init=None) -> dict:
        """kmeans(n_cells, iters, init) followed by set_partition(its centres, its assignment), as one unit on this handle ->
        partition_info()."""
        with self._call_lock:
            out = self.kmeans(n_cells, iters=iters, init=init)
            self.set_partition(out["centres"], out["assign"])
            return self.partition_info()

    def query_probed(self, queries, k: int, nprobe: int, require=None, exclude=None):
        """The exact top-k among the rows of the nprobe cells whose centres are nearest to each query, and the tail
        (mmiss_index_query_probed) -> (labels int64 [Q,k], distances float32 [Q,k], counts int32 [Q], scanned int64 [Q]): the
        distance bits and the order of query(); with every cell probed, query()'s result. A row in an unprobed cell is not
        returned however near it is. scanned[q] = the rows looked at for query q. require / exclude as in query(). 1 <= k <=
        2040, nprobe >= 1 (above the cell count: every cell). numpy in -> numpy out, CUDA tensor in -> CUDA tensors out. No
        partition raises."""
        k, nprobe = int(k), int(nprobe)
        if not 1 <= k <= self.MAX_K:
            raise ValueError(f"k: 1 .. {self.MAX_K}, got {k}")
        if nprobe < 1:
            raise ValueError(f"nprobe: at least 1, got {nprobe}")
        q, (lab, dist, cnt) = self._prepare(queries, k)
        Q = int(q.shape[0])
        if Q < 1:
            raise ValueError("query_probed takes at least one query")
        masks = self._masks(q, require, exclude) or (None, None)
        if _is_torch(q) and q.is_cuda:
            import torch

            scanned = torch.empty((Q,), dtype=torch.int64, device=q.device)
        else:
            scanned = np.empty((Q,), dtype=np.int64)
        with self._call_lock:
            self._sync_stream(q)
            _lib.check(self._lib.mmiss_index_query_probed(self._h, _lib.ptr(q), Q, k, nprobe, _lib.ptr(masks[0]), _lib.ptr(masks[1]),
                                                          _lib.ptr(lab), _lib.ptr(dist), _lib.ptr(cnt), _lib.ptr(scanned)))
        return lab, dist, cnt, scanned

    # ------------------------------------------------------------------ subset search
    def query_subset(self, queries, k: int, labels, require=None, exclude=None):
        """The exact top-k among the rows whose labels are listed (mmiss_index_query_subset) -> (labels int64 [Q,k], distances
        float32 [Q,k], counts int32 [Q], matched int64 [Q]): the distance bits and the order of query(); with every stored label
        listed, query()'s result. A row outside the list is not returned however near it is. `labels`: int64 [n], numpy or a
        CUDA tensor (a CUDA list goes with CUDA queries); a label that is not stored is ignored, a repeated one counts once, the
        order means nothing, an empty list gives counts 0. matched[q] = the listed rows that exist, the same for every query.
        require / exclude as in query(). 1 <= k <= 2040, at least one query. numpy in -> numpy out, CUDA tensor in -> CUDA
        tensors out."""
        k = int(k)
        if not 1 <= k <= self.MAX_K:
            raise ValueError(f"k: 1 .. {self.MAX_K}, got {k}")
        if _is_torch(labels):
            import torch

            if labels.dtype.is_floating_point or labels.dtype == torch.bool or labels.dtype.is_complex:
                raise TypeError(f"labels: integers expected, got {labels.dtype}")
            cand = labels.to(torch.int64).reshape(-1).contiguous()
            if not cand.is_cuda:
                cand = cand.numpy()
        else:
            cand = np.asarray(labels)
            if cand.size and cand.dtype.kind not in "ui":
                raise TypeError(f"labels: integers expected, got {cand.dtype}")
            cand = np.ascontiguousarray(cand, dtype=np.int64).reshape(-1)
        n_cand = int(cand.shape[0])
        if n_cand > 2 ** 31 - 1:
            raise ValueError(f"labels: at most {2 ** 31 - 1}, got {n_cand}")
        q, (lab, dist, cnt) = self._prepare(queries, k)
        Q = int(q.shape[0])
        if Q < 1:
            raise ValueError("query_subset takes at least one query")
        on_device = _is_torch(q) and q.is_cuda
        if _is_torch(cand) and not on_device:
            raise ValueError("labels: a CUDA list goes with CUDA queries")
        masks = self._masks(q, require, exclude) or (None, None)
        if on_device:
            import torch

            matched = torch.empty((Q,), dtype=torch.int64, device=q.device)
        else:
            matched = np.empty((Q,), dtype=np.int64)
        with self._call_lock:
            self._sync_stream(q)
            _lib.check(self._lib.mmiss_index_query_subset(self._h, _lib.ptr(q), Q, k, _lib.ptr(cand) if n_cand else None, n_cand,
                                                          _lib.ptr(masks[0]), _lib.ptr(masks[1]), _lib.ptr(lab), _lib.ptr(dist),
                                                          _lib.ptr(cnt), _lib.ptr(matched)))
        return lab, dist, cnt, matched

    # ------------------------------------------------------------------ search after
    @staticmethod
    def _per_query(x, Q: int, dtype, name: str):
        """x as a contiguous [Q] array of `dtype` (a numpy dtype): a CUDA tensor stays one, anything else becomes numpy; a scalar
        is repeated for every query."""
        if _is_torch(x) and x.is_cuda:
            import torch

            t = x.to(getattr(torch, np.dtype(dtype).name)).reshape(-1).contiguous()
            if t.shape[0] == 1 and Q > 1:
                t = t.expand(Q).contiguous()
            v = t
        else:
            if _is_torch(x):
                x = x.numpy()
            a = np.asarray(x)
            if np.dtype(dtype).kind == "i" and a.size and a.dtype.kind not in "ui":
                raise TypeError(f"{name}: integers expected, got {a.dtype}")
            a = a.astype(dtype).reshape(-1)
            if a.shape[0] == 1 and Q > 1:
                a = np.repeat(a, Q)
            v = np.ascontiguousarray(a)
        if int(v.shape[0]) != Q:
            raise ValueError(f"{name}: one value per query ({Q}) expected, got {int(v.shape[0])}")
        return v

    def query_after(self, queries, k: int, after_dist, after_label, max_dist=None, labels=None, require=None, exclude=None):
        """The exact next k of every query's ranking behind its cursor (mmiss_index_query_after) -> (labels int64 [Q,k], distances
        float32 [Q,k], counts int32 [Q], remaining int64 [Q]). The ranking is query()'s: canonical distance bits, ties by label.
        after_dist float32 [Q] / after_label int64 [Q]: the last entry the caller holds — a row is returned when its distance is
        larger (by the ranking's order of the bits), or equal with a larger label; -inf starts the ranking, NaN admits nothing,
        the label need not be stored. max_dist [Q] (None: none): only rows with distance <= it. labels (None: every row): only
        rows whose labels are listed, as query_subset's list; an empty list gives counts 0. require / exclude as in query().
        remaining[q]: the rows behind the cursor, those delivered included — 0 means the ranking has ended, remaining == count
        that this page is the last. Nothing is kept between calls. Scalars are repeated for every query. 1 <= k <= 2040, at
        least one query. numpy in -> numpy out, CUDA tensor in -> CUDA tensors out."""
        k = int(k)
        if not 1 <= k <= self.MAX_K:
            raise ValueError(f"k: 1 .. {self.MAX_K}, got {k}")
        cand, n_cand = None, 0
        if labels is not None:
            if _is_torch(labels):
                import torch

                if labels.dtype.is_floating_point or labels.dtype == torch.bool or labels.dtype.is_complex:
                    raise TypeError(f"labels: integers expected, got {labels.dtype}")
                cand = labels.to(torch.int64).reshape(-1).contiguous()
                if not cand.is_cuda:
                    cand = cand.numpy()
            else:
                cand = np.asarray(labels)
                if cand.size and cand.dtype.kind not in "ui":
                    raise TypeError(f"labels: integers expected, got {cand.dtype}")
                cand = np.ascontiguousarray(cand, dtype=np.int64).reshape(-1)
            n_cand = int(cand.shape[0])
            if n_cand > 2 ** 31 - 1:
                raise ValueError(f"labels: at most {2 ** 31 - 1}, got {n_cand}")
            if n_cand == 0:
                cand = np.zeros((1,), dtype=np.int64)   # the empty list is a non-null pointer with n_cand = 0
        q, (lab, dist, cnt) = self._prepare(queries, k)
        Q = int(q.shape[0])
        if Q < 1:
            raise ValueError("query_after takes at least one query")
        on_device = _is_torch(q) and q.is_cuda
        ad = self._per_query(after_dist, Q, np.float32, "after_dist")
        al = self._per_query(after_label, Q, np.int64, "after_label")
        md = None if max_dist is None else self._per_query(max_dist, Q, np.float32, "max_dist")
        if not on_device and any(_is_torch(v) for v in (ad, al, md, cand)):
            raise ValueError("CUDA cursors, radii and labels go with CUDA queries")
        masks = self._masks(q, require, exclude) or (None, None)
        if on_device:
            import torch

            remaining = torch.empty((Q,), dtype=torch.int64, device=q.device)
        else:
            remaining = np.empty((Q,), dtype=np.int64)
        with self._call_lock:
            self._sync_stream(q)
            _lib.check(self._lib.mmiss_index_query_after(self._h, _lib.ptr(q), Q, k, _lib.ptr(ad), _lib.ptr(al),
                                                         None if md is None else _lib.ptr(md), None if cand is None else _lib.ptr(cand),
                                                         n_cand, _lib.ptr(masks[0]), _lib.ptr(masks[1]), _lib.ptr(lab), _lib.ptr(dist),
                                                         _lib.ptr(cnt), _lib.ptr(remaining)))
        return lab, dist, cnt, remaining

    def ranking(self, query, n: int, page: int = 1000, **same):
        """The first n entries of ONE query's ranking, for any n, by chaining pages of query_after -> (labels int64 [m], distances
        float32 [m]), m <= n: it stops when a page comes back short. page: entries per call, 1 .. 2040. **same: the max_dist,
        labels, require and exclude of query_after, the same on every page."""
        n, page = int(n), int(page)
        if n < 0:
            raise ValueError(f"n: at least 0, got {n}")
        if not 1 <= page <= self.MAX_K:
            raise ValueError(f"page: 1 .. {self.MAX_K}, got {page}")
        on_device = _is_torch(query) and query.is_cuda
        q = query.reshape(1, -1) if _is_torch(query) else np.asarray(query, dtype=np.float32).reshape(1, -1)
        labs, dists = [], []
        ad, al = np.float32(-np.inf), np.int64(0)
        got = 0
        while got < n:
            k = min(page, n - got)
            lab, dist, cnt, _ = self.query_after(q, k, ad, al, **same)
            c = int(cnt[0])
            labs.append(lab[0, :c])
            dists.append(dist[0, :c])
            got += c
            if c < k:
                break
            ad, al = dist[0, c - 1:c], lab[0, c - 1:c]   # (views: a CUDA page's cursor stays on the device)
        if on_device:
            import torch

            if not labs:
                return (torch.empty((0,), dtype=torch.int64, device=query.device), torch.empty((0,), dtype=torch.float32, device=query.device))
            return torch.cat(labs), torch.cat(dists)
        if not labs:
            return np.empty((0,), np.int64), np.empty((0,), np.float32)
        return np.concatenate(labs), np.concatenate(dists)

    # ------------------------------------------------------------------ distinct results
    MAX_POOL = MAX_POOL

    def query_distinct(self, queries, k: int, min_sep: float, pool: Optional[int] = None, nprobe: int = 0, require=None, exclude=None):
        """Top-k with near-duplicates of kept hits suppressed on the device (mmiss_index_query_distinct) -> (labels int64 [Q,k],
        distances float32 [Q,k], counts int32 [Q], dups int32 [Q,k], listed int32 [Q]). The greedy walk over the exact ranked list
        of `pool` entries — query()'s, or with nprobe >= 1 query_probed()'s: an entry is suppressed when an earlier KEPT entry lies
        within cosine distance min_sep of it (the distance query_radius_by_label reports with the kept label as the query), else
        kept while fewer than k are. dups[q, j] = the list entries kept entry j owns, listed[q] = the list's length. The kept
        entries do not depend on pool once counts == k; counts < k with listed == pool means the pool ran out. pool None:
        min(2040, max(8 k, 64)). 1 <= k <= pool <= 2040; min_sep must not be NaN (negative: nothing is suppressed). require /
        exclude as in query(). numpy in -> numpy out, CUDA tensor in -> CUDA tensors out."""
        k, nprobe = int(k), int(nprobe)
        pool = default_distinct_pool(k) if pool is None else int(pool)
        min_sep = float(min_sep)
        if k < 1:
            raise ValueError(f"k: at least 1, got {k}")
        if not k <= pool <= self.MAX_POOL:
            raise ValueError(f"pool: k .. {self.MAX_POOL}, got {pool} (k = {k})")
        if min_sep != min_sep:
            raise ValueError("min_sep is NaN")
        if nprobe < 0:
            raise ValueError(f"nprobe: 0 (the flat list) or at least 1, got {nprobe}")
        q, (lab, dist, cnt) = self._prepare(queries, k)
        Q = int(q.shape[0])
        masks = self._masks(q, require, exclude) or (None, None)
        if _is_torch(q) and q.is_cuda:
            import torch

            dups = torch.empty((Q, k), dtype=torch.int32, device=q.device)
            listed = torch.empty((Q,), dtype=torch.int32, device=q.device)
        else:
            dups = np.empty((Q, k), dtype=np.int32)
            listed = np.empty((Q,), dtype=np.int32)
        with self._call_lock:
            self._sync_stream(q)
            _lib.check(self._lib.mmiss_index_query_distinct(self._h, _lib.ptr(q), Q, k, pool, min_sep, nprobe, _lib.ptr(masks[0]),
                                                            _lib.ptr(masks[1]), _lib.ptr(lab), _lib.ptr(dist), _lib.ptr(cnt), _lib.ptr(dups),
                                                            _lib.ptr(listed)))
        return lab, dist, cnt, dups, listed

    # ------------------------------------------------------------------ grouped search
    MAX_GROUPS = MAX_GROUPS

    def set_groups(self, labels, groups) -> None:
        """Per-row int32 GROUP (mmiss_index_set_groups): labels [n], groups [n], -1 <= group < MAX_GROUPS; -1 = no group (the row
        is a group of its own). A label not in the index or a value outside the range raises and changes nothing. Rows are added
        with -1; update keeps a row's group; removal keeps the survivors'; clear and load reset every group to -1."""
        lab = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
        g = np.asarray(groups)
        if g.dtype.kind not in "ui" and not (g.dtype == object and g.size == 0):
            raise TypeError(f"groups must be integers, got {g.dtype}")
        g = g.reshape(-1)
        if g.shape[0] != lab.shape[0]:
            raise ValueError(f"{lab.shape[0]} labels but {g.shape[0]} groups")
        if g.size and (int(g.min()) < -1 or int(g.max()) >= self.MAX_GROUPS):
            raise ValueError(f"groups: -1 .. {self.MAX_GROUPS - 1}, got {int(g.min())} .. {int(g.max())}")
        g = np.ascontiguousarray(g, dtype=np.int32)
        with self._call_lock:
            _lib.check(self._lib.mmiss_index_set_groups(self._h, lab.ctypes.data, g.ctypes.data, int(lab.shape[0])))

    def get_groups(self, labels) -> np.ndarray:
        """-> int32 [n], the groups of `labels` (a label not in the index raises)."""
        lab = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
        out = np.full(lab.shape[0], -1, dtype=np.int32)
        if lab.shape[0]:
            with self._call_lock:
                _lib.check(self._lib.mmiss_index_get_groups(self._h, lab.ctypes.data, int(lab.shape[0]), out.ctypes.data))
        return out

    def query_grouped(self, queries, k: int, pool: Optional[int] = None, require=None, exclude=None):
        """The exact k nearest GROUPS, each by its best row (mmiss_index_query_grouped) -> (labels int64 [Q,k], distances float32
        [Q,k], groups int32 [Q,k], counts int32 [Q], route int32 [Q]): the first k group heads of the complete ranking query()
        would give over all admitted rows, a row without a group counting as a group of its own; groups[q, j] = the head's group
        (-1: none, and behind the count). Exact at any group size and independent of `pool`: route[q] = 0 when the walk over the
        top-`pool` list answered, 1 when one group owned the pool and the query was answered by the scan of every row. pool None:
        min(2040, max(8 k, 64)); else k <= pool <= 2040. 1 <= k <= 2040, at least one query. require / exclude as in query().
        numpy in -> numpy out, CUDA tensor in -> CUDA tensors out."""
        k = int(k)
        if not 1 <= k <= self.MAX_K:
            raise ValueError(f"k: 1 .. {self.MAX_K}, got {k}")
        pool = 0 if pool is None else int(pool)
        if pool != 0 and not k <= pool <= self.MAX_POOL:
            raise ValueError(f"pool: k .. {self.MAX_POOL}, got {pool} (k = {k})")
        q, (lab, dist, cnt) = self._prepare(queries, k)
        Q = int(q.shape[0])
        if Q < 1:
            raise ValueError("query_grouped takes at least one query")
        masks = self._masks(q, require, exclude) or (None, None)
        if _is_torch(q) and q.is_cuda:
            import torch

            grp = torch.empty((Q, k), dtype=torch.int32, device=q.device)
            route = torch.empty((Q,), dtype=torch.int32, device=q.device)
        else:
            grp = np.empty((Q, k), dtype=np.int32)
            route = np.empty((Q,), dtype=np.int32)
        with self._call_lock:
            self._sync_stream(q)
            _lib.check(self._lib.mmiss_index_query_grouped(self._h, _lib.ptr(q), Q, k, pool, _lib.ptr(masks[0]), _lib.ptr(masks[1]),
                                                           _lib.ptr(lab), _lib.ptr(dist), _lib.ptr(grp), _lib.ptr(cnt), _lib.ptr(route)))
        return lab, dist, grp, cnt, route

    def guard_stats(self) -> dict:
        """Exactness accounting (mmiss_index_guard_stats_ex): queries served, queries whose first pass could not be proven
        exact and were widened, widen (threshold) passes run, extra passes over the index they cost, the queries that ended in
        the exhaustive canonical pass (a tie plateau of more than 8192 rows), the rows the threshold passes re-ranked, and the
        radius calls' own two: the queries they served and the passes over the index those cost. membership() / tag_by_radius()
        count like radius calls: their probes and passes, the (row, probe) pairs they resolved canonically under swept_rows, the
        probes that took the per-probe canonical route under exhaustive. assign() counts its centres and passes there too, and
        borderline rows x centres with a direction under swept_rows."""
        out = (C.c_int64 * 8)()
        _lib.check(self._lib.mmiss_index_guard_stats_ex(self._h, out))
        return {"queries": out[0], "widened": out[1], "rounds": out[2], "pages": out[3], "exhaustive": out[4],
                "swept_rows": out[5], "radius_queries": out[6], "radius_pages": out[7]}

    # ------------------------------------------------------------------ persistence
    def save(self, path: str) -> None:
        _lib.check(self._lib.mmiss_index_save(self._h, str(path).encode()))

    def load(self, path: str) -> None:
        _lib.check(self._lib.mmiss_index_load(self._h, str(path).encode()))

    def abort_query(self) -> None:
        """Drop a query opened with query_begin() whose handle was lost (mmiss_index_query_abort); no-op otherwise."""
        with self._call_lock:
            self._query_gen += 1   # whatever handle held the open query is stale from here on
            _lib.check(self._lib.mmiss_index_query_abort(self._h))

    def close(self):
        if getattr(self, "_h", None):
            with self._call_lock:
                self._query_gen += 1
                self._lib.mmiss_index_query_abort(self._h)   # (an abandoned PendingQuery must not outlive its buffers)
                self._lib.mmiss_index_destroy(self._h)
                self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PendingQuery:
    """A query between FlatIndex.query_begin and its result(): holds the query rows and the output buffers alive. It owns the
    index's open-query slot only while its generation is the index's current one (FlatIndex._query_gen)."""

    def __init__(self, index: "FlatIndex", q, outs, gen: int, masks=None):
        self._index, self._q, self._outs, self._gen, self._done = index, q, outs, gen, False
        self._masks = masks   # (read by the begin call already; kept with the query for symmetry with `q`)

    def _current(self) -> bool:
        idx = self._index
        return getattr(idx, "_h", None) is not None and idx._query_gen == self._gen

    def result(self):
        if not self._done:
            idx = self._index
            with idx._call_lock:
                if not self._current():
                    self._done = True
                    self._q = None
                    raise RuntimeError("this query was aborted (FlatIndex.abort_query / close, or a later query_begin)")
                self._done = True   # (whatever _end returns, the C side has closed the query)
                idx._query_gen += 1
                _lib.check(idx._lib.mmiss_index_query_end(idx._h))
            self._q = None
        return self._outs

    def abort(self) -> None:
        """Give the query up (mmiss_index_query_abort): waits for the queued first pass, delivers nothing, frees the index
        for other calls. Also what happens when the handle is dropped or leaves a `with` block without result(). A handle
        whose query is no longer the index's open one (already aborted through the index, or superseded) does nothing."""
        if not self._done:
            self._done = True
            idx = self._index
            with idx._call_lock:
                if self._current():
                    idx._query_gen += 1
                    idx._lib.mmiss_index_query_abort(idx._h)
            self._q = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.abort()
        return False

    def __del__(self):
        try:
            self.abort()
        except Exception:
            pass


def blend(img, txt, weight_image: float, device: int = 0):
    """normalize(w * normalize(img) + (1 - w) * normalize(txt)) row-wise — backend/app/main.py:852-860."""
    lib = _lib.load()
    if _is_torch(img) and img.is_cuda:
        import torch

        img = img.to(torch.float32).contiguous()
        txt = txt.to(torch.float32).contiguous()
        out = torch.empty_like(img)
        stream = _lib.current_stream_ptr(img.device)
        device = img.device.index if img.device.index is not None else device
    else:
        img = np.ascontiguousarray(img, dtype=np.float32)
        txt = np.ascontiguousarray(txt, dtype=np.float32)
        out = np.empty_like(img)
        stream = None
    one_d = img.ndim == 1
    Q = 1 if one_d else int(img.shape[0])
    D = int(img.shape[-1])
    if tuple(img.shape) != tuple(txt.shape):
        raise ValueError("image and text embeddings differ in shape")
    _lib.check(lib.mmiss_blend(device, stream, _lib.ptr(img), _lib.ptr(txt), float(weight_image), Q, D, _lib.ptr(out)))
    return out


def merge_topk(dist, labels, device: int = 0):
    """dist [S,Q,k] f32, labels [S,Q,k] i64 (per-shard results) -> (labels [Q,k], dist [Q,k], count [Q])."""
    lib = _lib.load()
    S, Q, k = (int(x) for x in dist.shape)
    if _is_torch(dist) and dist.is_cuda:
        import torch

        dist = dist.contiguous()
        labels = labels.contiguous()
        od = torch.empty((Q, k), dtype=torch.float32, device=dist.device)
        ol = torch.empty((Q, k), dtype=torch.int64, device=dist.device)
        oc = torch.empty((Q,), dtype=torch.int32, device=dist.device)
        stream = _lib.current_stream_ptr(dist.device)
        device = dist.device.index if dist.device.index is not None else device
    else:
        dist = np.ascontiguousarray(dist, dtype=np.float32)
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        od = np.empty((Q, k), dtype=np.float32)
        ol = np.empty((Q, k), dtype=np.int64)
        oc = np.empty((Q,), dtype=np.int32)
        stream = None
    _lib.check(lib.mmiss_merge_topk(device, stream, _lib.ptr(dist), _lib.ptr(labels), S, Q, k, _lib.ptr(od), _lib.ptr(ol), _lib.ptr(oc)))
    return ol, od, oc
