"""FlatCollection — the chromadb Collection surface the reference uses, over the in-HBM FlatIndex.

Call sites mirrored (paths relative to the reference root):
  client.create_collection(name, metadata={"hnsw:space": "cosine"})     backend/app/utils.py:127-130
  collection.add(ids, embeddings, metadatas, documents)                  backend/app/main.py:735-740
  collection.query(query_embeddings, n_results, include)                 backend/app/main.py:761-765
  collection.get(ids=..., include=[...]) / get(include=[])               backend/app/main.py:533,556,563-566,631-634
  collection.update(ids, metadatas)                                      backend/app/main.py:503-510,1030-1033
  collection.delete(ids)                                                 backend/app/main.py:1065-1069
  collection.count()                                                     init_db.py:58

Filtered search (query(..., filters=[names])) is exact PRE-filtering: the top-k among the rows whose filter_results_json
answers "yes" to every named filter, where the reference post-filters the k nearest rows (backend/app/main.py:202-222) and
so returns fewer. Each filter name gets one bit of the index rows' 64-bit tag words (FlatIndex.set_tags), in order of first
appearance in label order; the bits are derived from the metadata, never persisted, and pushed to the index lazily — at
the first filtered query after the metadata changed.

Only the embedding arithmetic runs on the GPU (FlatIndex); ids, metadatas and documents are host-side
bookkeeping exactly as they are bookkeeping inside chromadb's sqlite. String ids map to int64 labels
handed out in insertion order; labels are the deterministic tie-break of equal distances.
"""
from __future__ import annotations

import json
import logging
import os
import re
import threading
from typing import Dict, List, Optional, Sequence

import numpy as np

from .index import MAX_GROUPS, MAX_POOL, FlatIndex, default_distinct_pool

logger = logging.getLogger("image-match")
MAX_N_RESULTS = 2040  # mmiss_index_query's per-call limit on k
MAX_FILTER_BITS = 64  # bits of a row's tag word (mmiss_index_set_tags)


def filter_answers(metadata) -> dict:
    """The yes/no answers of one row: its metadata's `filter_results_json` parsed (unparseable or not an object: none)."""
    if not metadata or "filter_results_json" not in metadata:
        return {}
    try:
        answers = json.loads(metadata["filter_results_json"])
    except (json.JSONDecodeError, TypeError):
        return {}
    return answers if isinstance(answers, dict) else {}


def answers_yes(value) -> bool:
    """The normalisation of api.apply_filters (backend/app/main.py:216-218)."""
    return str(value).lower().strip() == "yes"


_WHERE_COMPARE = {
    "$eq": lambda a, b: a == b, "$ne": lambda a, b: a != b,
    "$gt": lambda a, b: a > b, "$gte": lambda a, b: a >= b, "$lt": lambda a, b: a < b, "$lte": lambda a, b: a <= b,
    "$in": lambda a, b: a in b, "$nin": lambda a, b: a not in b,
}


def check_where(where) -> None:
    """Raise ValueError unless `where` is a predicate where_matches evaluates: {"field": value}, {"field": {"$op": operand}} with
    $eq $ne $gt $gte $lt $lte $in $nin, {"$and": [predicates]}, {"$or": [predicates]}; several keys of one dict all have to hold."""
    if not isinstance(where, dict) or not where:
        raise ValueError(f"where: a non-empty dict expected, got {where!r}")
    for key, cond in where.items():
        if key in ("$and", "$or"):
            if not isinstance(cond, (list, tuple)) or not cond:
                raise ValueError(f"where: {key} takes a non-empty list of predicates")
            for sub in cond:
                check_where(sub)
        elif not isinstance(key, str) or key.startswith("$"):
            raise ValueError(f"where: unknown operator {key!r}")
        elif isinstance(cond, dict):
            if not cond:
                raise ValueError(f"where: no operator for field {key!r}")
            for op, operand in cond.items():
                if op not in _WHERE_COMPARE:
                    raise ValueError(f"where: unknown operator {op!r}")
                if op in ("$in", "$nin") and not isinstance(operand, (list, tuple, set, frozenset)):
                    raise ValueError(f"where: {op} takes a list of values")
        elif isinstance(cond, (list, tuple, set)):
            raise ValueError(f"where: field {key!r} compared with {type(cond).__name__}; use $in")


def where_matches(metadata, where) -> bool:
    """Does one row's metadata satisfy `where` (checked by check_where)? A row without the field matches only $ne / $nin; values
    that do not compare ($gt between a string and a number) do not match."""
    metadata = metadata or {}
    for key, cond in where.items():
        if key == "$and":
            ok = all(where_matches(metadata, sub) for sub in cond)
        elif key == "$or":
            ok = any(where_matches(metadata, sub) for sub in cond)
        else:
            ok = True
            for op, operand in (cond.items() if isinstance(cond, dict) else (("$eq", cond),)):
                if key not in metadata:
                    ok = op in ("$ne", "$nin")
                else:
                    try:
                        ok = bool(_WHERE_COMPARE[op](metadata[key], operand))
                    except TypeError:
                        ok = False
                if not ok:
                    break
        if not ok:
            return False
    return True


_TOKEN = re.compile(r"^([0-9a-f]{8})\.(-?[0-9]{1,19})$")


def make_token(distance, label: int) -> str:
    """The continuation token of a result entry: the float32 distance's bits and the row's label, "%08x.%d". Opaque to callers."""
    return "%08x.%d" % (int(np.asarray(distance, dtype=np.float32).view(np.uint32)), int(label))


def parse_token(token) -> tuple:
    """make_token's inverse -> (distance float32, label int); anything else raises ValueError."""
    m = _TOKEN.match(token) if isinstance(token, str) else None
    if m is None or not -2 ** 63 <= int(m.group(2)) < 2 ** 63:
        raise ValueError(f"after: not a continuation token: {token!r}")
    return np.array([int(m.group(1), 16)], dtype=np.uint32).view(np.float32)[0], int(m.group(2))


class DuplicateIDError(ValueError):
    """Same condition chromadb reports for add() of an id that already exists."""


def _as_list(x):
    if x is None:
        return None
    if isinstance(x, (str, bytes)):
        return [x]
    return list(x)


class FlatCollection:
    def __init__(self, name: str = "image-match", dim: Optional[int] = None, dtype: str = "f32", device: int = 0,
                 metadata: Optional[dict] = None, persist_dir: Optional[str] = None, autosave: bool = True):
        self.name = name
        self.metadata = dict(metadata or {"hnsw:space": "cosine"})
        space = self.metadata.get("hnsw:space", "cosine")
        if space != "cosine":
            raise ValueError(f"FlatCollection implements the cosine space only (got {space!r})")
        self._dim = dim
        self._dtype = dtype
        self._device = device
        self._index: Optional[FlatIndex] = None
        self._ids: List[str] = []              # row order == label order
        self._labels: List[int] = []
        self._by_id: Dict[str, int] = {}       # id -> label
        self._meta: Dict[int, Optional[dict]] = {}
        self._docs: Dict[int, Optional[str]] = {}
        self._next_label = 0
        # filtered search: filter name -> tag bit, names answered past the 64th bit, labels whose tags the index does not have yet
        self._filter_bits: Dict[str, int] = {}
        self._filter_overflow: set = set()
        self._tag_dirty: set = set()
        # grouped search: the metadata field the index's groups stand for, its values' dense ids (order of first appearance, by
        # label), labels whose group the index does not have yet, rows per value (None: to be counted again)
        self._group_field: Optional[str] = None
        self._group_ids: Dict[tuple, int] = {}
        self._group_dirty: set = set()
        self._group_sizes: Optional[Dict[tuple, int]] = None
        self._lock = threading.RLock()         # 1 writer + readers (the reference has a background updater, main.py:410)
        self._persist_dir = persist_dir
        self._autosave = autosave
        if persist_dir:
            os.makedirs(persist_dir, exist_ok=True)
            if os.path.exists(self._meta_path()):
                self._load()

    # ------------------------------------------------------------------ persistence (replaces chroma_data/)
    def _meta_path(self):
        return os.path.join(self._persist_dir, f"{self.name}.meta.json")

    def _index_path(self, gen: int = 0):
        """Generation 0 is the legacy single-file name; later generations carry their number, and the metadata file
        names the generation it belongs to - so replacing the metadata file is the one atomic switch of a save."""
        suffix = "" if gen == 0 else f".{gen}"
        return os.path.join(self._persist_dir, f"{self.name}.index{suffix}.mmiss")

    def _journal_paths(self, gen: int):
        base = os.path.join(self._persist_dir, f"{self.name}.journal.{gen}")
        return base + ".jsonl", base + ".f32"

    def persist(self) -> None:
        """Full snapshot (compaction): metadata file + a new index generation; the journal of the previous generation is
        dropped. O(N) — called on create, explicitly, and automatically when the journal has grown past a quarter of the
        collection (see _saved): ordinary add / update / delete only append to the journal."""
        if not self._persist_dir:
            return
        with self._lock:
            old_gen = getattr(self, "_index_gen", 0)
            new_gen = old_gen + 1
            blob = {
                "name": self.name, "metadata": self.metadata, "dim": self._dim, "dtype": self._dtype,
                "next_label": self._next_label, "ids": self._ids, "labels": self._labels,
                "metadatas": [self._meta.get(l) for l in self._labels],
                "documents": [self._docs.get(l) for l in self._labels],
                "index_gen": new_gen,
            }
            tmp = self._meta_path() + ".tmp"
            with open(tmp, "w") as f:
                json.dump(blob, f)
                f.flush()
                os.fsync(f.fileno())
            if self._index is not None:
                self._index.save(self._index_path(new_gen))   # a new file: the previous generation stays intact
            os.replace(tmp, self._meta_path())                 # the atomic switch
            self._index_gen = new_gen
            self._journal_rows = 0
            for path in (self._index_path(old_gen),) + self._journal_paths(old_gen):
                try:
                    os.remove(path)
                except FileNotFoundError:
                    pass

    def _journal(self, record: dict, vectors: Optional[np.ndarray] = None) -> None:
        """Append one mutation to the journal of the current generation: the vectors (raw float32, as handed to add /
        update — replay re-normalises them, bit-identically) first, then ONE json line that is the commit record. O(batch),
        where a full snapshot per uploaded image would be O(N) (10 GB per /api/upload at 10M x 512 f16)."""
        jl, jv = self._journal_paths(getattr(self, "_index_gen", 0))
        if vectors is not None:
            with open(jv, "ab") as f:
                record["offset"] = f.tell()
                record["rows"] = int(vectors.shape[0])
                record["dim"] = int(vectors.shape[1])
                f.write(np.ascontiguousarray(vectors, dtype=np.float32).tobytes())
                f.flush()
                os.fsync(f.fileno())
        with open(jl, "a") as f:
            f.write(json.dumps(record) + "\n")
            f.flush()
            os.fsync(f.fileno())
        self._journal_rows = getattr(self, "_journal_rows", 0) + max(1, len(record.get("ids", [])))

    def _replay_journal(self) -> None:
        jl, jv = self._journal_paths(self._index_gen)
        if not os.path.exists(jl):
            # No commit line exists in this generation. A crash inside the FIRST journaled mutation's vector write still leaves
            # bytes in the vector file that no record owns: drop them, or the next add records an offset behind (or inside)
            # them and the restart after that one cuts the whole log back to nothing.
            if os.path.exists(jv) and os.path.getsize(jv) > 0:
                with open(jv, "r+b") as f:
                    f.truncate(0)
                    f.flush()
                    os.fsync(f.fileno())
            return
        # The vector file may end in a torn write (a crash inside f.write of the vectors — the large write, so the likelier one
        # to tear): its size need not be a multiple of 4. Map only the whole floats; the tail is cut off below.
        vec_bytes = os.path.getsize(jv) if os.path.exists(jv) else 0
        vec = np.memmap(jv, dtype=np.float32, mode="r", shape=(vec_bytes // 4,)) if vec_bytes >= 4 else None
        vec_end = 0           # byte offset just behind the last committed record's vectors
        autosave, self._autosave = self._autosave, False   # replay must not journal again
        good_end = 0          # byte offset just behind the last committed record
        torn = needs_newline = False
        try:
            with open(jl, "rb") as f:
                for raw in f:
                    try:
                        rec = json.loads(raw.decode("utf-8"))
                        if not isinstance(rec, dict) or "op" not in rec:
                            raise ValueError("not a journal record")
                    except ValueError:
                        torn = True                          # a torn last line: the mutation was never committed
                        break
                    emb = None
                    if "offset" in rec:
                        o, n, d = rec["offset"] // 4, rec["rows"], rec["dim"]
                        if vec is None or (o + n * d) > vec.shape[0]:
                            torn = True                      # the commit line survived, its vectors did not: not committed
                            break
                        if rec["offset"] % 4:
                            torn = True                      # (written behind a torn tail by a build without the cut below)
                            break
                        emb = np.array(vec[o:o + n * d]).reshape(n, d)
                        vec_end = max(vec_end, (o + n * d) * 4)
                    if rec["op"] == "add":
                        self.add(rec["ids"], emb, rec.get("metadatas"), rec.get("documents"))
                    elif rec["op"] == "update":
                        self.update(rec["ids"], emb, rec.get("metadatas"), rec.get("documents"), _replace_metadata=True)
                    elif rec["op"] == "delete":
                        self.delete(rec["ids"])
                    self._journal_rows = getattr(self, "_journal_rows", 0) + max(1, len(rec.get("ids", [])))
                    good_end += len(raw)
                    needs_newline = not raw.endswith(b"\n")   # (a complete record whose newline was cut off)
        finally:
            self._autosave = autosave
        # Leave the file ending in a newline behind the last committed record: later appends would otherwise be glued to
        # the torn bytes, become unparsable, and every mutation acknowledged after the crash would be lost at the next restart.
        if torn or needs_newline:
            with open(jl, "r+b") as f:
                f.truncate(good_end)
                if needs_newline:
                    f.seek(good_end)
                    f.write(b"\n")
                f.flush()
                os.fsync(f.fileno())
        # ... and the vector file ending behind the last committed record's vectors: the next append records f.tell() as its
        # offset, which must be 4-aligned and must not sit behind bytes no record owns.
        if vec_bytes > vec_end:
            del vec
            with open(jv, "r+b") as f:
                f.truncate(vec_end)
                f.flush()
                os.fsync(f.fileno())

    def _load(self) -> None:
        with open(self._meta_path()) as f:
            blob = json.load(f)
        self.metadata = blob.get("metadata", self.metadata)
        self._dim = blob["dim"]
        self._dtype = blob.get("dtype", self._dtype)
        self._next_label = blob["next_label"]
        self._ids = list(blob["ids"])
        self._labels = [int(x) for x in blob["labels"]]
        self._by_id = dict(zip(self._ids, self._labels))
        self._meta = dict(zip(self._labels, blob["metadatas"]))
        self._docs = dict(zip(self._labels, blob["documents"]))
        self._index_gen = int(blob.get("index_gen", 0))
        # the index file holds no tags (they load as 0): every row's tag is pushed again at the first filtered query
        self._filter_bits, self._filter_overflow, self._tag_dirty = {}, set(), set(self._labels)
        # ... and no groups (they load as -1): the field is mapped and pushed again at the first grouped query
        self._group_field, self._group_ids, self._group_dirty, self._group_sizes = None, {}, set(), None
        if self._dim is not None and self._labels:
            self._ensure_index(self._dim)
            self._index.load(self._index_path(self._index_gen))
            if self._index.count() != len(self._labels):
                raise RuntimeError("collection files are inconsistent (row count differs from id count)")
        self._journal_rows = 0
        self._replay_journal()

    def _saved(self, record: Optional[dict] = None, vectors: Optional[np.ndarray] = None):
        """After a mutation (called under the lock): append it to the journal; compact into a full snapshot once the
        journal holds more than max(4096, a quarter of the collection) rows."""
        if not (self._autosave and self._persist_dir):
            return
        if record is None:
            self.persist()
            return
        self._journal(record, vectors)
        if self._journal_rows > max(4096, len(self._ids) // 4):
            self.persist()

    # ------------------------------------------------------------------ helpers
    def _ensure_index(self, dim: int) -> FlatIndex:
        if self._index is None:
            self._dim = int(dim)
            self._index = FlatIndex(self._dim, self._dtype, self._device)
        elif dim != self._dim:
            raise ValueError(f"embedding dimension {dim} does not match the collection's {self._dim}")
        return self._index

    @staticmethod
    def _embeddings_array(embeddings) -> np.ndarray:
        arr = np.asarray(embeddings, dtype=np.float32)
        if arr.ndim == 1:
            arr = arr[None]
        if arr.ndim != 2:
            raise ValueError("embeddings must be a list of vectors")
        return np.ascontiguousarray(arr)

    # ------------------------------------------------------------------ chroma surface
    def count(self) -> int:
        with self._lock:
            return len(self._ids)

    def add(self, ids, embeddings, metadatas=None, documents=None) -> None:
        ids = _as_list(ids)
        emb = self._embeddings_array(embeddings)  # the reference passes python lists of floats (main.py:687)
        metadatas = _as_list(metadatas) if metadatas is not None else [None] * len(ids)
        documents = _as_list(documents) if documents is not None else [None] * len(ids)
        if not (len(ids) == emb.shape[0] == len(metadatas) == len(documents)):
            raise ValueError("ids, embeddings, metadatas and documents differ in length")
        with self._lock:
            if len(set(ids)) != len(ids):
                raise DuplicateIDError("duplicate ids in add()")
            dup = [i for i in ids if i in self._by_id]
            if dup:
                raise DuplicateIDError(f"ids already in collection: {dup[:3]}")
            index = self._ensure_index(emb.shape[1])
            labels = np.arange(self._next_label, self._next_label + len(ids), dtype=np.int64)
            index.add(emb, labels)
            self._next_label += len(ids)
            for i, lab in zip(ids, labels.tolist()):
                self._ids.append(i)
                self._labels.append(lab)
                self._by_id[i] = lab
            for lab, m, d in zip(labels.tolist(), metadatas, documents):
                self._meta[lab] = dict(m) if m is not None else None
                self._docs[lab] = d
            self._tag_dirty.update(labels.tolist())
            self._group_dirty.update(labels.tolist())
            self._group_sizes = None
            self._saved({"op": "add", "ids": ids, "metadatas": metadatas, "documents": documents}, emb)

    # ------------------------------------------------------------------ filtered search
    def _push_tags(self) -> None:
        """Give the index the tag words of every dirty label (under the lock, at a filtered query). Labels are visited in label
        order, so a name's bit is the order of its first appearance."""
        if not self._tag_dirty:
            return
        labs = sorted(self._tag_dirty)
        tags = []
        for lab in labs:
            t = 0
            for name, value in filter_answers(self._meta.get(lab)).items():
                bit = self._filter_bits.get(name)
                if bit is None and name not in self._filter_overflow:
                    if len(self._filter_bits) < MAX_FILTER_BITS:
                        bit = self._filter_bits[name] = len(self._filter_bits)
                    else:
                        self._filter_overflow.add(name)
                if bit is not None and answers_yes(value):
                    t |= 1 << bit
            tags.append(t)
        self._index.set_tags(np.asarray(labs, dtype=np.int64), np.asarray(tags, dtype=np.uint64))
        self._tag_dirty.clear()

    def _index_query(self, q: np.ndarray, k: int, max_distance=None, n_probe=None, **masks):
        """The index's top-k query or, max_distance given, its radius query with k as the cap (FlatIndex.query_radius: only the
        rows within max_distance, the k nearest of them) -> (labels [Q,k], distances [Q,k], counts [Q]). n_probe given, no
        max_distance and a partition present: the probed query (FlatIndex.query_probed) instead of the flat one."""
        if max_distance is None:
            if n_probe is not None and self._index.partition_info()["cells"] > 0:
                return self._index.query_probed(q, k, int(n_probe), **masks)[:3]
            return self._index.query(q, k, **masks)
        return self._index.query_radius(q, max_distance, k, **masks)[:3]

    def _filtered_query(self, q: np.ndarray, k: int, filters: List[str], max_distance=None, n_probe=None):
        """Exact top-k among the rows answering "yes" to every filter -> (labels [Q,k], distances [Q,k], counts [Q]);
        max_distance: among those of them within that distance."""
        self._push_tags()
        Q = q.shape[0]
        if any(f not in self._filter_bits and f not in self._filter_overflow for f in filters):
            # a name no row has ever answered admits nothing
            return (np.full((Q, k), -1, np.int64), np.full((Q, k), np.inf, np.float32), np.zeros((Q,), np.int32))
        req = 0
        for f in filters:
            if f in self._filter_bits:
                req |= 1 << self._filter_bits[f]
        over = [f for f in filters if f in self._filter_overflow]
        if not over:
            return self._index_query(q, k, max_distance, n_probe, require=np.uint64(req))
        # a name past the 64th bit: the mapped bits narrow the query, the rest is checked on the host. Exact as long as the rows
        # passing the mapped bits fit one call (MAX_N_RESULTS); beyond that it is the best MAX_N_RESULTS of them, post-filtered.
        ok = {lab for lab in self._labels if all(answers_yes(filter_answers(self._meta.get(lab)).get(f, "")) for f in filters)}
        wide = min(len(self._labels), MAX_N_RESULTS)
        labs_w, dist_w, cnt_w = self._index_query(q, wide, max_distance, require=np.uint64(req))
        labs = np.full((Q, k), -1, np.int64)
        dist = np.full((Q, k), np.inf, np.float32)
        cnt = np.zeros((Q,), np.int32)
        for qi in range(Q):
            keep = [j for j in range(int(cnt_w[qi])) if int(labs_w[qi, j]) in ok][:k]
            labs[qi, :len(keep)] = labs_w[qi, keep]
            dist[qi, :len(keep)] = dist_w[qi, keep]
            cnt[qi] = len(keep)
        return labs, dist, cnt

    def _distinct_query(self, q: np.ndarray, k: int, filters: List[str], distinct_distance: float, pool: Optional[int],
                        max_distance=None, n_probe=None):
        """The distinct top-k (FlatIndex.query_distinct) among the rows answering "yes" to every filter -> (labels [Q,k], distances
        [Q,k], counts [Q], dups [Q,k]). A query whose pool ran out (count < k, listed == pool) below the largest pool repeats the
        call once at the largest: sound, because the kept entries for a pool are a prefix of those for any larger one.
        max_distance cuts the kept list at the radius: the ranking is sorted by distance, so the cut is a prefix."""
        Q = q.shape[0]
        masks = {}
        if filters:
            self._push_tags()
            over = [f for f in filters if f in self._filter_overflow]
            if over:
                raise ValueError(f"distinct_distance cannot be combined with filter names past the {MAX_FILTER_BITS}th ({over[:3]}): "
                                 "the host post-filter would change which images count as kept")
            if any(f not in self._filter_bits for f in filters):   # a name no row has ever answered admits nothing
                return (np.full((Q, k), -1, np.int64), np.full((Q, k), np.inf, np.float32), np.zeros((Q,), np.int32),
                        np.zeros((Q, k), np.int32))
            req = 0
            for f in filters:
                req |= 1 << self._filter_bits[f]
            masks = {"require": np.uint64(req)}
        nprobe = int(n_probe) if n_probe is not None and self._index.partition_info()["cells"] > 0 else 0
        pool = default_distinct_pool(k) if pool is None else min(max(int(pool), k), MAX_POOL)
        labs, dist, cnt, dups, listed = self._index.query_distinct(q, k, distinct_distance, pool, nprobe, **masks)
        if pool < MAX_POOL and bool(((np.asarray(cnt) < k) & (np.asarray(listed) == pool)).any()):
            labs, dist, cnt, dups, listed = self._index.query_distinct(q, k, distinct_distance, MAX_POOL, nprobe, **masks)
        labs, dist, cnt, dups = np.asarray(labs), np.asarray(dist), np.array(cnt, np.int32), np.asarray(dups)
        if max_distance is not None:
            within = (dist <= np.float32(max_distance)) & (np.arange(k)[None, :] < cnt[:, None])
            cnt = within.sum(1).astype(np.int32)
        return labs, dist, cnt, dups

    # ------------------------------------------------------------------ grouped search
    @staticmethod
    def _group_key(metadata, field: str):
        """the value of `field` in a row's metadata as a dictionary key (1, 1.0, True and "1" are different groups), None when the
        row has no such field"""
        v = (metadata or {}).get(field)
        return None if v is None else (type(v).__name__, v)

    def _push_groups(self, field: str) -> None:
        """Give the index the group of every dirty label (under the lock, at a grouped query); another field than the last one's
        maps its values afresh and pushes every label. Labels are visited in label order, so a value's id is the order of its
        first appearance. A row without the field is ungrouped (-1)."""
        if field != self._group_field:
            self._group_field, self._group_ids, self._group_sizes = field, {}, None
            self._group_dirty = set(self._labels)
        if not self._group_dirty:
            return
        labs = sorted(self._group_dirty)
        groups = []
        for lab in labs:
            key = self._group_key(self._meta.get(lab), field)
            if key is None:
                groups.append(-1)
                continue
            gid = self._group_ids.get(key)
            if gid is None:
                if len(self._group_ids) >= MAX_GROUPS:
                    raise ValueError(f"group_by: more than {MAX_GROUPS} different values of {field!r}")
                gid = self._group_ids[key] = len(self._group_ids)
            groups.append(gid)
        self._index.set_groups(np.asarray(labs, dtype=np.int64), np.asarray(groups, dtype=np.int32))
        self._group_dirty.clear()

    def _group_counts(self, field: str) -> Dict[tuple, int]:
        """stored rows per value of the field, from the host metadata; counted once per state of the collection"""
        if self._group_sizes is None:
            sizes: Dict[tuple, int] = {}
            for lab in self._labels:
                key = self._group_key(self._meta.get(lab), field)
                if key is not None:
                    sizes[key] = sizes.get(key, 0) + 1
            self._group_sizes = sizes
        return self._group_sizes

    def _grouped_query(self, q: np.ndarray, k: int, field: str, filters: List[str], pool: Optional[int], max_distance=None):
        """The k nearest groups of `field`, each by its best row (FlatIndex.query_grouped), among the rows answering "yes" to every
        filter -> (labels [Q,k], distances [Q,k], counts [Q]). max_distance cuts the heads at the radius: they are sorted by
        distance, and a group has a row within the radius exactly if its head is, so the cut is a prefix."""
        Q = q.shape[0]
        self._push_groups(field)
        masks = {}
        if filters:
            self._push_tags()
            over = [f for f in filters if f in self._filter_overflow]
            if over:
                raise ValueError(f"group_by cannot be combined with filter names past the {MAX_FILTER_BITS}th ({over[:3]}): "
                                 "the host post-filter would change which image stands for a group")
            if any(f not in self._filter_bits for f in filters):   # a name no row has ever answered admits nothing
                return np.full((Q, k), -1, np.int64), np.full((Q, k), np.inf, np.float32), np.zeros((Q,), np.int32)
            req = 0
            for f in filters:
                req |= 1 << self._filter_bits[f]
            masks = {"require": np.uint64(req)}
        pool = None if pool is None else min(max(int(pool), k), MAX_POOL)
        labs, dist, _grp, cnt, _route = self._index.query_grouped(q, k, pool, **masks)
        labs, dist, cnt = np.asarray(labs), np.asarray(dist), np.array(cnt, np.int32)
        if max_distance is not None:
            within = (dist <= np.float32(max_distance)) & (np.arange(k)[None, :] < cnt[:, None])
            cnt = within.sum(1).astype(np.int32)
        return labs, dist, cnt

    def _admitted_labels(self, ids, where) -> List[int]:
        """The labels `ids` (chroma ids; unknown ones are ignored; None: every row) and `where` (a metadata predicate, None: every
        row) admit, in label order."""
        if ids is None:
            labs = self._labels
        else:
            labs = sorted({self._by_id[i] for i in _as_list(ids) if i in self._by_id})
        if where is not None:
            labs = [lab for lab in labs if where_matches(self._meta.get(lab), where)]
        return list(labs)

    def _subset_query(self, q: np.ndarray, k: int, labs: List[int], filters: List[str], max_distance=None):
        """Exact top-k among the rows `labs` that answer "yes" to every filter (FlatIndex.query_subset) -> (labels [Q,k], distances
        [Q,k], counts [Q]). Up to 64 filter names travel as masks; a name past the 64th bit is folded into the list on the host,
        which stays exact at any size. max_distance cuts the sorted result at the radius: a prefix."""
        Q = q.shape[0]
        empty = (np.full((Q, k), -1, np.int64), np.full((Q, k), np.inf, np.float32), np.zeros((Q,), np.int32))
        masks = {}
        if filters:
            self._push_tags()
            if any(f not in self._filter_bits and f not in self._filter_overflow for f in filters):
                return empty                                             # a name no row has ever answered admits nothing
            req = 0
            for f in filters:
                if f in self._filter_bits:
                    req |= 1 << self._filter_bits[f]
            if req:
                masks = {"require": np.uint64(req)}
            over = [f for f in filters if f in self._filter_overflow]
            if over:
                labs = [lab for lab in labs if all(answers_yes(filter_answers(self._meta.get(lab)).get(f, "")) for f in over)]
        if not labs:
            return empty
        labs_o, dist, cnt, _ = self._index.query_subset(q, k, np.asarray(labs, dtype=np.int64), **masks)
        labs_o, dist, cnt = np.asarray(labs_o), np.asarray(dist), np.array(cnt, np.int32)
        if max_distance is not None:
            within = (dist <= np.float32(max_distance)) & (np.arange(k)[None, :] < cnt[:, None])
            cnt = within.sum(1).astype(np.int32)
        return labs_o, dist, cnt

    def _after_query(self, q: np.ndarray, k: int, cursors, labs, filters: List[str], max_distance=None):
        """The exact next k of every query's ranking behind its cursor (FlatIndex.query_after) -> (labels [Q,k], distances [Q,k],
        counts [Q], remaining [Q]). cursors: (distance, label) per query; labs: the admitted labels, None for every row. Filters
        travel as _subset_query's do: up to 64 names as masks, a name past the 64th bit folded into the list on the host."""
        Q = q.shape[0]
        empty = (np.full((Q, k), -1, np.int64), np.full((Q, k), np.inf, np.float32), np.zeros((Q,), np.int32), np.zeros((Q,), np.int64))
        kw = {}
        if filters:
            self._push_tags()
            if any(f not in self._filter_bits and f not in self._filter_overflow for f in filters):
                return empty                                             # a name no row has ever answered admits nothing
            req = 0
            for f in filters:
                if f in self._filter_bits:
                    req |= 1 << self._filter_bits[f]
            if req:
                kw["require"] = np.uint64(req)
            over = [f for f in filters if f in self._filter_overflow]
            if over:
                labs = [lab for lab in (self._labels if labs is None else labs)
                        if all(answers_yes(filter_answers(self._meta.get(lab)).get(f, "")) for f in over)]
        if labs is not None:
            if not labs:
                return empty
            kw["labels"] = np.asarray(labs, dtype=np.int64)
        if max_distance is not None:
            kw["max_dist"] = np.full((Q,), max_distance, dtype=np.float32)
        ad = np.array([c[0] for c in cursors], dtype=np.float32)
        al = np.array([c[1] for c in cursors], dtype=np.int64)
        labs_o, dist, cnt, rem = self._index.query_after(q, k, ad, al, **kw)
        return np.asarray(labs_o), np.asarray(dist), np.array(cnt, np.int32), np.array(rem, np.int64)

    def query(self, query_embeddings=None, n_results: int = 10, include: Sequence[str] = ("metadatas", "documents", "distances"),
              filters: Optional[Sequence[str]] = None, max_distance: Optional[float] = None, n_probe: Optional[int] = None,
              distinct_distance: Optional[float] = None, pool: Optional[int] = None, ids=None, where: Optional[dict] = None,
              after: Optional[Sequence[Optional[str]]] = None, group_by: Optional[str] = None, **_unused) -> dict:
        """collection.query. filters: names of yes/no filters; when given, the result is the exact n_results nearest among the
        rows whose filter_results_json answers "yes" to every one of them (pre-filtering; see the module docstring).
        max_distance: a radius query (FlatIndex.query_radius) — only the rows within that cosine distance are returned, exactly,
        and n_results is the cap on how many (the nearest ones). It combines with filters: the members among the rows the filters
        admit; past 64 filter names the host post-filter of the filtered query applies to the radius result (the best
        MAX_N_RESULTS members passing the mapped bits, post-filtered).
        n_probe: with a partition present (build_partition), search only the n_probe cells nearest to each query and the rows
        added since (FlatIndex.query_probed): the exact n_results nearest among those rows, filters included (up to 64 filter
        names). Without a partition, with max_distance, or with more than 64 filter names it is ignored: the exact answer, never
        an error.
        distinct_distance: suppress near-duplicates of kept results (FlatIndex.query_distinct): walking the exact ranking, a row
        within that cosine distance of an earlier KEPT result is dropped and counted under that result; n_results different
        images come back, and the dict gains "duplicates" — per query, the rows each result stands for besides itself. pool:
        how much of the ranking is walked (None: min(2040, max(8 n_results, 64)); a query that runs out is repeated once at
        2040). Works with filters (up to 64 names; a name past the 64th raises ValueError), n_probe and max_distance (the kept
        list cut at the radius). Without distinct_distance nothing changes.
        ids / where (chromadb's collection.query(ids=, where=)): search only among these rows — `ids` chroma ids (unknown ones are
        ignored), `where` a metadata predicate ({"field": v}, $eq $ne $gt $gte $lt $lte $in $nin, $and, $or; anything else raises
        ValueError; a row without the field matches only $ne / $nin); both given: their intersection. The result is the exact
        n_results nearest among the admitted rows (FlatIndex.query_subset), at any size of the list. filters combine (up to 64
        names as masks, names past the 64th folded into the list: exact, where the filtered query's host post-filter is not),
        max_distance cuts the sorted result at the radius, n_probe is ignored (the subset is exact), distinct_distance raises
        ValueError, an empty admitted set gives empty results. Without ids and where nothing changes.
        after: continue a ranking ("show more"; FlatIndex.query_after) — one entry per query, the "next" token of the page the
        caller holds, or None for the start of the ranking; a malformed token raises ValueError. The result is the exact
        n_results entries that follow that one (up to 2040 per call; no warning), at a cost that does not grow with the depth,
        and the dict gains "next" (per query: the token of the last entry, None when this page is the last) and "remaining" (per
        query: the rows behind the cursor, this page's included). Tokens are opaque and hold no state: rows added or removed
        between two pages are ranked as they stand. filters (masks; names past the 64th folded into the list), ids / where (the
        list) and max_distance combine and must be the same on every page; n_probe is ignored (the continuation is exact);
        distinct_distance raises ValueError. Without after nothing changes.
        group_by: the n_results nearest GROUPS, one hit each (FlatIndex.query_grouped) — a group is the rows whose metadata field
        `group_by` has the same value (a folder, an album, an upload batch, a cluster), a row without the field is a group of its
        own; each group is represented by its nearest row, at any group size (one group holding the nearest 5000 rows costs a scan
        of the index, not the result). The dict gains "groups" (per query and result: the field's value, None for a row without
        the field) and "group_sizes" (the stored rows with that value, from the metadata; 1 for a row without the field). filters
        combine (up to 64 names as masks; a name past the 64th raises ValueError), max_distance cuts the heads at the radius,
        pool is how much of the ranking is walked before the scan takes over (it never changes the result); ids / where / after /
        distinct_distance / n_probe raise ValueError. Without group_by nothing changes.
        Nothing is written, neither metadata nor journal."""
        if n_probe is not None and int(n_probe) < 1:
            raise ValueError(f"n_probe: at least 1, got {n_probe}")
        if group_by is not None:
            if not isinstance(group_by, str) or not group_by:
                raise ValueError(f"group_by: the name of a metadata field expected, got {group_by!r}")
            for name, given in (("ids", ids), ("where", where), ("after", after), ("distinct_distance", distinct_distance), ("n_probe", n_probe)):
                if given is not None:
                    raise ValueError(f"group_by cannot be combined with {name}")
        subset = ids is not None or where is not None
        if where is not None:
            check_where(where)
        if subset and distinct_distance is not None:
            raise ValueError("distinct_distance cannot be combined with ids / where")
        cursors = None
        if after is not None:
            if distinct_distance is not None:
                raise ValueError("distinct_distance cannot be combined with after")
            if isinstance(after, str):
                raise ValueError("after: a list with one entry per query expected")
            cursors = [(np.float32(-np.inf), 0) if t is None else parse_token(t) for t in after]
        if distinct_distance is not None:
            distinct_distance = float(distinct_distance)
            if distinct_distance != distinct_distance:
                raise ValueError("distinct_distance is NaN")
        dups = None
        filters = list(dict.fromkeys(_as_list(filters))) if filters else []
        if query_embeddings is None:
            raise ValueError("FlatCollection.query needs query_embeddings (text embedding functions are out of scope)")
        q = self._embeddings_array(query_embeddings)
        include = list(include)
        if cursors is not None and len(cursors) != q.shape[0]:
            raise ValueError(f"after: one entry per query ({q.shape[0]}) expected, got {len(cursors)}")
        with self._lock:
            Q = q.shape[0]
            n = len(self._ids)
            rem = np.zeros((Q,), dtype=np.int64)
            if n == 0 or self._index is None:
                labs = np.full((Q, 0), -1, dtype=np.int64)
                dist = np.zeros((Q, 0), dtype=np.float32)
                cnt = np.zeros((Q,), dtype=np.int32)
            elif cursors is not None:
                if q.shape[1] != self._dim:
                    raise ValueError(f"query dimension {q.shape[1]} does not match the collection's {self._dim}")
                k = max(1, min(int(n_results), n, MAX_N_RESULTS))
                labs, dist, cnt, rem = self._after_query(q, k, cursors, self._admitted_labels(ids, where) if subset else None,
                                                         filters, max_distance)
            else:
                if q.shape[1] != self._dim:
                    raise ValueError(f"query dimension {q.shape[1]} does not match the collection's {self._dim}")
                k = max(1, min(int(n_results), n))  # n_results > count is not an error ("All" = 1000, main.py:757)
                if k > MAX_N_RESULTS:  # one mmiss_index_query call ranks at most 2040 rows per query: clamp, do not fail
                    logger.warning(f"n_results={n_results} clamped to {MAX_N_RESULTS}")
                    k = MAX_N_RESULTS
                if group_by is not None:
                    labs, dist, cnt = self._grouped_query(q, k, group_by, filters, pool, max_distance)
                elif subset:
                    labs, dist, cnt = self._subset_query(q, k, self._admitted_labels(ids, where), filters, max_distance)
                elif distinct_distance is not None:
                    labs, dist, cnt, dups = self._distinct_query(q, k, filters, distinct_distance, pool, max_distance, n_probe)
                elif filters:
                    labs, dist, cnt = self._filtered_query(q, k, filters, max_distance, n_probe)
                else:
                    labs, dist, cnt = self._index_query(q, k, max_distance, n_probe)
            label_to_id = dict(zip(self._labels, self._ids))
            out = {"ids": [], "distances": None, "metadatas": None, "documents": None, "embeddings": None,
                   "uris": None, "data": None, "included": include}
            rows = []
            for qi in range(Q):
                ls = [int(x) for x in labs[qi, : int(cnt[qi])]]
                rows.append(ls)
                out["ids"].append([label_to_id[l] for l in ls])
            if "distances" in include:
                out["distances"] = [[float(x) for x in dist[qi, : int(cnt[qi])]] for qi in range(Q)]
            if "metadatas" in include:
                out["metadatas"] = [[self._meta.get(l) for l in ls] for ls in rows]
            if "documents" in include:
                out["documents"] = [[self._docs.get(l) for l in ls] for ls in rows]
            if "embeddings" in include:
                out["embeddings"] = [self._index.get(np.asarray(ls, dtype=np.int64)) for ls in rows]
            if distinct_distance is not None:
                out["duplicates"] = [[] if dups is None else [int(x) for x in dups[qi, : int(cnt[qi])]] for qi in range(Q)]
            if group_by is not None:
                sizes = self._group_counts(group_by) if rows and any(rows) else {}
                keys = [[self._group_key(self._meta.get(l), group_by) for l in ls] for ls in rows]
                out["groups"] = [[None if key is None else key[1] for key in ks] for ks in keys]
                out["group_sizes"] = [[1 if key is None else sizes.get(key, 0) for key in ks] for ks in keys]
            if cursors is not None:
                out["remaining"] = [int(r) for r in rem]
                out["next"] = [make_token(dist[qi, int(cnt[qi]) - 1], labs[qi, int(cnt[qi]) - 1]) if int(rem[qi]) > int(cnt[qi]) else None
                               for qi in range(Q)]
            return out

    def add_similarity_filter(self, name: str, embedding, max_distance: float) -> int:
        """A yes/no filter answered by the embedding arithmetic itself: every stored row gets "yes" under `name` in its
        filter_results_json when it lies within cosine distance max_distance of `embedding` (exactly: the member definition of
        FlatIndex.query_radius), "no" otherwise -> the number of "yes" rows. The CLIP form of the reference's add_filter ->
        process_filter_on_all_images (backend/app/main.py:939-1056), which asks a yes/no model about every image and stores
        the answers the searches filter on (main.py:202-222).
        ONE FlatIndex.membership call decides all rows (the only GPU work); writing the answers is a walk over the metadata of
        every row on the host, proportional to count(), through this collection's own update(): journaled, and the rows' tag
        words are re-derived from the metadata at the next filtered query — the metadata stays the source of truth for them, so
        query(filters=[name]), api.apply_filters, persistence and more than 64 filter names work as for any other answer.
        Answers other filters left in filter_results_json are kept. Rows added later have no answer under `name` (as the
        reference's filters until it processes them); running the filter again refreshes every row."""
        name = str(name)
        q = self._embeddings_array(embedding)
        if q.shape[0] != 1:
            raise ValueError("add_similarity_filter takes one embedding")
        with self._lock:
            if not self._ids or self._index is None:
                return 0
            if q.shape[1] != self._dim:
                raise ValueError(f"embedding dimension {q.shape[1]} does not match the collection's {self._dim}")
            words, members = self._index.membership(q, float(max_distance))
            words = np.asarray(words.cpu() if hasattr(words, "cpu") else words)
            if words.shape[0] != len(self._labels):
                raise RuntimeError("index and collection differ in row count")
            yes = (words.astype(np.uint64) & np.uint64(1)).astype(bool)   # row order == label order == self._labels
            metas = []
            for lab, y in zip(self._labels, yes.tolist()):
                answers = dict(filter_answers(self._meta.get(lab)))
                answers[name] = "yes" if y else "no"
                metas.append({"filter_results_json": json.dumps(answers)})
            self.update(ids=list(self._ids), metadatas=metas)
            return int(yes.sum())

    def assign(self, embeddings) -> tuple:
        """For EVERY stored row, the nearest of the given embeddings (FlatIndex.assign: smallest cosine distance, ties to the
        smaller index) -> (ids, assign int32 [count], dist float32 [count], sizes int64 [C]): ids[r] is the id of row r, assign[r]
        the index of its embedding (-1 and +inf for a row without a direction), sizes[c] the rows that chose embedding c. One
        call on the index; nothing is written, neither metadata nor journal. embeddings: [C, dim], 1 <= C <= 1024."""
        c = self._embeddings_array(embeddings)
        with self._lock:
            if c.shape[0] < 1:
                raise ValueError("assign takes at least one embedding")
            if not self._ids or self._index is None:
                return [], np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(c.shape[0], np.int64)
            if c.shape[1] != self._dim:
                raise ValueError(f"embedding dimension {c.shape[1]} does not match the collection's {self._dim}")
            a, d, sizes = self._index.assign(c)
            if int(np.asarray(a).shape[0]) != len(self._labels):
                raise RuntimeError("index and collection differ in row count")
            return list(self._ids), np.asarray(a), np.asarray(d), np.asarray(sizes)    # (row order == label order == self._ids)

    def cluster(self, n_clusters: int, iters: int = 10, init_ids=None) -> dict:
        """Spherical k-means over the stored rows (FlatIndex.kmeans, deterministic) -> its dict plus "ids": ids[r] is the id of
        row r of "assign" / "dist". init_ids: the ids of the n_clusters rows to start from (None: rows spread evenly over the
        collection). Nothing is written."""
        with self._lock:
            if not self._ids or self._index is None:
                raise ValueError("cluster on an empty collection")
            init = None
            if init_ids is not None:
                id_to_label = dict(zip(self._ids, self._labels))
                init = np.asarray([id_to_label[i] for i in init_ids], dtype=np.int64)
            out = dict(self._index.kmeans(int(n_clusters), iters=int(iters), init=init))
            if int(np.asarray(out["assign"]).shape[0]) != len(self._labels):
                raise RuntimeError("index and collection differ in row count")
            out["ids"] = list(self._ids)
            return out

    def build_partition(self, n_cells: int, iters: int = 10) -> dict:
        """Partition the stored rows into n_cells k-means cells for query(..., n_probe=) (FlatIndex.build_partition) -> its info
        dict. Rows added afterwards are searched by every probed query; update and delete drop the partition (queries then run
        flat until it is built again), and it is not persisted. Nothing is written."""
        with self._lock:
            if not self._ids or self._index is None:
                raise ValueError("build_partition on an empty collection")
            return self._index.build_partition(int(n_cells), iters=int(iters))

    def partition_info(self) -> dict:
        """FlatIndex.partition_info of the collection's index; "cells" = 0 when there is no partition (or no index yet)."""
        with self._lock:
            if self._index is None:
                return {"cells": 0, "rows": 0, "tail": 0, "rows_in_cells": 0, "largest_cell": 0, "empty_cells": 0, "queries": 0, "scanned": 0}
            return self._index.partition_info()

    def near_duplicates(self, max_distance: float, cap_per_row: int = 64) -> List[tuple]:
        """Every pair of stored rows within cosine distance max_distance, each once (FlatIndex.near_duplicates) ->
        [(id_a, id_b, distance)], id_a the row added earlier, ordered by (id_a's position, distance, id_b's position); a row
        with more than cap_per_row later partners reports its cap_per_row nearest."""
        with self._lock:
            if not self._ids or self._index is None:
                return []
            a, b, d = self._index.near_duplicates(max_distance, cap_per_row)[:3]
            label_to_id = dict(zip(self._labels, self._ids))
            return [(label_to_id[int(x)], label_to_id[int(y)], float(z)) for x, y, z in zip(a, b, d)]

    def get(self, ids=None, include: Sequence[str] = ("metadatas", "documents"), limit: Optional[int] = None,
            offset: Optional[int] = None, where: Optional[dict] = None, **_unused) -> dict:
        """collection.get. where: the metadata predicate of query(where=), applied before offset and limit."""
        include = list(include)
        if where is not None:
            check_where(where)
        with self._lock:
            if ids is None:
                sel = list(zip(self._ids, self._labels))
            else:
                sel = [(i, self._by_id[i]) for i in _as_list(ids) if i in self._by_id]  # missing ids are skipped
            if where is not None:
                sel = [(i, l) for i, l in sel if where_matches(self._meta.get(l), where)]
            if offset:
                sel = sel[int(offset):]
            if limit is not None:
                sel = sel[: int(limit)]
            out = {"ids": [i for i, _ in sel], "metadatas": None, "documents": None, "embeddings": None,
                   "uris": None, "data": None, "included": include}
            if "metadatas" in include:
                out["metadatas"] = [self._meta.get(l) for _, l in sel]
            if "documents" in include:
                out["documents"] = [self._docs.get(l) for _, l in sel]
            if "embeddings" in include:
                labs = np.asarray([l for _, l in sel], dtype=np.int64)
                out["embeddings"] = self._index.get(labs) if (self._index is not None and labs.size) else np.zeros((0, self._dim or 0), np.float32)
            return out

    def update(self, ids, embeddings=None, metadatas=None, documents=None, _replace_metadata: bool = False) -> None:
        ids = _as_list(ids)
        with self._lock:
            missing = [i for i in ids if i not in self._by_id]
            if missing:
                raise ValueError(f"ids not in collection: {missing[:3]}")
            labs = [self._by_id[i] for i in ids]
            if metadatas is not None:
                for lab, m in zip(labs, _as_list(metadatas)):
                    if m is not None:
                        merged = {} if _replace_metadata else dict(self._meta.get(lab) or {})
                        merged.update(m)  # chroma merges keys on update
                        self._meta[lab] = merged
                        self._tag_dirty.add(lab)
                        self._group_dirty.add(lab)
                        self._group_sizes = None
            if documents is not None:
                for lab, d in zip(labs, _as_list(documents)):
                    self._docs[lab] = d
            emb = None
            if embeddings is not None:
                emb = self._embeddings_array(embeddings)
                self._index.update(np.asarray(labs, dtype=np.int64), emb)
            # the journal records the RESULTING metadata (replay replaces instead of merging: idempotent)
            self._saved({"op": "update", "ids": ids,
                         "metadatas": [self._meta.get(l) for l in labs] if metadatas is not None else None,
                         "documents": [self._docs.get(l) for l in labs] if documents is not None else None}, emb)

    def delete(self, ids=None) -> None:
        with self._lock:
            if ids is None:
                ids = list(self._ids)
            ids = [i for i in _as_list(ids) if i in self._by_id]
            if not ids:
                return
            labs = [self._by_id[i] for i in ids]
            self._index.remove(np.asarray(labs, dtype=np.int64))
            gone = set(labs)
            keep = [(i, l) for i, l in zip(self._ids, self._labels) if l not in gone]
            self._ids = [i for i, _ in keep]
            self._labels = [l for _, l in keep]
            for i, l in zip(ids, labs):
                del self._by_id[i]
                self._meta.pop(l, None)
                self._docs.pop(l, None)
                self._tag_dirty.discard(l)
                self._group_dirty.discard(l)
            self._group_sizes = None
            self._saved({"op": "delete", "ids": ids})

    def peek(self, limit: int = 10) -> dict:
        return self.get(limit=limit)


class PersistentClient:
    """Minimal stand-in for chromadb.PersistentClient(path) as the reference drives it (utils.py:113-130)."""

    def __init__(self, path: str = "chroma_data", device: int = 0, dtype: str = "f32"):
        self.path = path
        self.device = device
        self.dtype = dtype
        os.makedirs(path, exist_ok=True)
        self._open: Dict[str, FlatCollection] = {}

    def list_collections(self) -> List[str]:
        names = {n[: -len(".meta.json")] for n in os.listdir(self.path) if n.endswith(".meta.json")}
        return sorted(names | set(self._open))

    def get_collection(self, name: str) -> FlatCollection:
        if name in self._open:
            return self._open[name]
        if name not in self.list_collections():
            raise ValueError(f"Collection {name} does not exist.")
        col = FlatCollection(name, persist_dir=self.path, device=self.device, dtype=self.dtype)
        self._open[name] = col
        return col

    def create_collection(self, name: str, metadata: Optional[dict] = None) -> FlatCollection:
        if name in self.list_collections():
            raise ValueError(f"Collection {name} already exists.")
        col = FlatCollection(name, metadata=metadata, persist_dir=self.path, device=self.device, dtype=self.dtype)
        col.persist()
        self._open[name] = col
        return col

    def get_or_create_collection(self, name: str, metadata: Optional[dict] = None) -> FlatCollection:
        return self.get_collection(name) if name in self.list_collections() else self.create_collection(name, metadata)

    def delete_collection(self, name: str) -> None:
        self._open.pop(name, None)
        for fn in os.listdir(self.path):   # the metadata file and every index generation of this collection
            if fn == name + ".meta.json" or fn == name + ".meta.json.tmp" or (
                    fn.startswith(name + ".index") and fn.endswith(".mmiss")) or fn.startswith(name + ".journal."):
                os.remove(os.path.join(self.path, fn))
