"""Host-side mirror of the search / ingest orchestration on the hot path of the reference's
backend/app/main.py (same names, argument meaning, return layout and error behaviour):

  search_similar(embedding, limit)                             main.py:748-805
  search_by_text(query_text, limit)                            main.py:807-827
  search_multimodal(image, query_text, weight_image, limit)    main.py:829-867
  process_image(...) — the embedding + collection.add portion  main.py:685-687,733-744
  apply_text_filter(filter_query, min_similarity) /            main.py:939-1056 (add_filter -> process_filter_on_all_images),
  apply_image_filter(image, name, min_similarity)              answered by CLIP similarity instead of a yes/no model
  classify_collection(prompts) / cluster_collection(n)         no counterpart: CLIP's zero-shot classification of every stored
                                                               image, and k-means albums, in the index's own arithmetic

plus batched forms (the reference is batch-1 everywhere; BASELINE configs 2-4 are batched).
Like the reference, the wrappers catch every exception, log it and return [].
Every search takes a keyword-only `filters` (names of yes/no filters): the exact `limit` nearest among the images that answer
"yes" to all of them (FlatCollection.query(filters=...)); the default None searches everything, as the reference does.
Every search also takes `distinct_similarity`: near-duplicates of kept results are suppressed on the device and counted.
Every search also takes `within_ids` (image ids) and `where` (a metadata predicate): the exact `limit` nearest among those images
only (FlatCollection.query(ids=, where=)) — an album, a folder, the hits of an earlier search.
Every search also takes `after`: "show more". "" asks for the first page, the "next" token of a page for the one behind it (one
entry per query for the batch forms); the call then returns {"results": [...], "next": token or None, "remaining": n} instead of the
bare list (the batch forms: one such dict per query) — the exact continuation of the ranking at any depth
(FlatCollection.query(after=)). The other arguments must be those of the page before. None (the default): today's call and list.
"""
from __future__ import annotations

import logging
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import utils
from .collection import DuplicateIDError
from .index import blend

logger = logging.getLogger("image-match")

# module-global collection, as in the reference (main.py:77,530)
collection = None


def set_collection(col) -> None:
    global collection
    collection = col


def _collection():
    global collection
    if collection is None:
        collection = utils.init_chromadb()
    return collection


def _results_from_query(results: dict, qi: int) -> List[Dict]:
    """main.py:768-801 for one query row."""
    similar_images = []
    if not results or "ids" not in results or not results["ids"]:
        return []
    result_ids = results["ids"][qi]
    result_metadatas = results["metadatas"][qi]
    result_distances = results["distances"][qi]
    result_duplicates = results["duplicates"][qi] if results.get("duplicates") is not None else None
    result_groups = results["groups"][qi] if results.get("groups") is not None else None
    # cosine distance: 0 = identical, 2 = opposite; similarity 1 = identical, 0 = opposite (main.py:782)
    similarities = [1 - (distance / 2) for distance in result_distances]
    for i, img_id in enumerate(result_ids):
        metadata = result_metadatas[i]
        result_metadata = metadata.copy() if metadata is not None else {}
        result_metadata["similarity_score"] = similarities[i]
        if result_duplicates is not None:
            result_metadata["duplicates"] = result_duplicates[i]
        if result_groups is not None:
            result_metadata["group"] = result_groups[i]
            result_metadata["group_size"] = results["group_sizes"][qi][i]
        if "url" not in result_metadata:
            result_metadata["url"] = f"/static/processed/{img_id}.png"
        if "thumbnail_url" not in result_metadata:
            result_metadata["thumbnail_url"] = f"/static/processed/{img_id}.png"
        similar_images.append(result_metadata)
    return similar_images


def _paged(results: dict, qi: int) -> Dict:
    """one query's page of a FlatCollection.query(after=) result"""
    return {"results": _results_from_query(results, qi), "next": results["next"][qi], "remaining": results["remaining"][qi]}


def _no_page() -> Dict:
    """what a paged search answers when it fails (the list forms answer [])"""
    return {"results": [], "next": None, "remaining": 0}


def _filter_kw(filters, min_similarity=None, n_probe=None, distinct_similarity=None, within_ids=None, where=None, after=None,
               group_by=None) -> dict:
    """the keyword arguments of FlatCollection.query for a search's filters, similarity threshold, probe count and distinctness;
    min_similarity = s becomes the radius utils.max_distance_for_similarity(s): on its results "similarity_score >= s" holds for
    exactly the members; distinct_similarity = s becomes distinct_distance the same way: a result at least s similar to an earlier
    kept result is dropped and counted under it"""
    kw = {"filters": list(filters)} if filters else {}
    if min_similarity is not None:
        kw["max_distance"] = float(utils.max_distance_for_similarity(min_similarity))
    if n_probe is not None:
        kw["n_probe"] = int(n_probe)
    if distinct_similarity is not None:
        kw["distinct_distance"] = float(utils.max_distance_for_similarity(distinct_similarity))
    # within_ids / where: search among these images only; absent, no argument at all (today's call)
    if within_ids is not None:
        kw["ids"] = [within_ids] if isinstance(within_ids, str) else list(within_ids)
    if where is not None:
        kw["where"] = where
    # after: one token per query, "" / None for the start of the ranking; absent, no argument at all (today's call)
    if after is not None:
        kw["after"] = [t or None for t in after]
    # group_by: one result per value of this metadata field; absent, no argument at all (today's call)
    if group_by is not None:
        kw["group_by"] = group_by
    return kw


def search_similar(embedding: np.ndarray, limit: int = 10, *, filters: Optional[Sequence[str]] = None,
                   min_similarity: Optional[float] = None, n_probe: Optional[int] = None,
                   distinct_similarity: Optional[float] = None, within_ids: Optional[Sequence[str]] = None,
                   where: Optional[dict] = None, after: Optional[str] = None, group_by: Optional[str] = None):
    """Search for similar images using an embedding (main.py:748-805). min_similarity: only the images whose similarity_score
    reaches it, exactly (a radius query; `limit` caps how many) — the reference's roadmap item "Adjustable similarity
    thresholds" (CHANGELOG.md:475). n_probe: search only the n_probe k-means cells nearest to the embedding, and what was added
    since (build_search_partition; FlatCollection.query(n_probe=)); without a partition the search is the exact one.
    distinct_similarity: `limit` DIFFERENT images — walking the ranking, an image at least that similar to an earlier kept result is
    dropped and counted under it; every result then carries "duplicates", the images it stands for besides itself
    (FlatCollection.query(distinct_distance=)).
    within_ids / where: only among these images — ids (unknown ones are ignored) and / or a metadata predicate; the exact `limit`
    nearest of them (FlatCollection.query(ids=, where=)); n_probe is then ignored, and distinct_similarity is refused (logged, []).
    after: "" for the first page, a page's "next" token for the one behind it -> {"results", "next", "remaining"} (module docstring);
    n_probe is then ignored; distinct_similarity and a malformed token are refused (logged, an empty page).
    group_by: the `limit` nearest GROUPS, one image each — a group is the images whose metadata field `group_by` has the same value
    (a folder, an upload batch), an image without the field is a group of its own; every result then carries "group" (the value,
    None without the field) and "group_size" (the stored images with that value) (FlatCollection.query(group_by=)). Combined with
    n_probe, distinct_similarity, within_ids, where or after it is refused (logged, [] or an empty page)."""
    try:
        actual_limit = 1000 if limit <= 0 else limit  # "All" option (limit of 0), main.py:757
        results = _collection().query(query_embeddings=[np.asarray(embedding, dtype=np.float32).tolist()],
                                      n_results=actual_limit, include=["metadatas", "distances"],
                                      **_filter_kw(filters, min_similarity, n_probe, distinct_similarity, within_ids, where,
                                                   None if after is None else [after], group_by))
        if after is not None:
            return _paged(results, 0)
        out = _results_from_query(results, 0)
        logger.info(f"Found {len(out)} similar images")
        return out
    except Exception as e:
        logger.error(f"Error searching for similar images: {e}")
        return [] if after is None else _no_page()


def search_similar_batch(embeddings: np.ndarray, limit: int = 10, *, filters: Optional[Sequence[str]] = None,
                         min_similarity: Optional[float] = None, n_probe: Optional[int] = None,
                         distinct_similarity: Optional[float] = None, within_ids: Optional[Sequence[str]] = None,
                         where: Optional[dict] = None, after: Optional[Sequence[Optional[str]]] = None,
                         group_by: Optional[str] = None):
    """[Q, D] embeddings -> one result list per query, one index pass for the whole batch. after: one entry per query ("" / None:
    the first page) -> one {"results", "next", "remaining"} per query."""
    try:
        actual_limit = 1000 if limit <= 0 else limit
        q = np.asarray(embeddings, dtype=np.float32)
        if after is not None and (isinstance(after, str) or len(after) != q.shape[0]):
            raise ValueError(f"after: one entry per query ({q.shape[0]}) expected")
        results = _collection().query(query_embeddings=q, n_results=actual_limit, include=["metadatas", "distances"],
                                      **_filter_kw(filters, min_similarity, n_probe, distinct_similarity, within_ids, where, after,
                                                   group_by))
        if after is not None:
            return [_paged(results, qi) for qi in range(q.shape[0])]
        return [_results_from_query(results, qi) for qi in range(q.shape[0])]
    except Exception as e:
        logger.error(f"Error searching for similar images: {e}")
        return []


def search_by_text(query_text: str, limit: int = 10, *, filters: Optional[Sequence[str]] = None,
                   min_similarity: Optional[float] = None, n_probe: Optional[int] = None,
                   distinct_similarity: Optional[float] = None, within_ids: Optional[Sequence[str]] = None,
                   where: Optional[dict] = None, after: Optional[str] = None, group_by: Optional[str] = None):
    """Search for images using a text query (main.py:807-827)."""
    try:
        model, processor = utils.load_clip_model()
        embedding_result = utils.generate_clip_embedding(text=query_text, model=model, processor=processor)
        text_embedding = embedding_result["text"][0]
        return search_similar(embedding=text_embedding, limit=limit, filters=filters, min_similarity=min_similarity, n_probe=n_probe,
                              distinct_similarity=distinct_similarity, within_ids=within_ids, where=where, after=after, group_by=group_by)
    except Exception as e:
        logger.error(f"Error in text search: {e}")
        return [] if after is None else _no_page()


def search_multimodal(image, query_text: str, weight_image: float = 0.5, limit: int = 10, *,
                      filters: Optional[Sequence[str]] = None, min_similarity: Optional[float] = None, n_probe: Optional[int] = None,
                      distinct_similarity: Optional[float] = None, within_ids: Optional[Sequence[str]] = None,
                      where: Optional[dict] = None, after: Optional[str] = None, group_by: Optional[str] = None):
    """Search using both image and text with a weighted combination (main.py:829-867); weight_image is not
    clamped, as in the backend route."""
    try:
        model, processor = utils.load_clip_model()
        image_embedding = utils.generate_clip_embedding(image=image, model=model, processor=processor)["image"][0]
        text_embedding = utils.generate_clip_embedding(text=query_text, model=model, processor=processor)["text"][0]
        # normalise both, weighted sum, normalise again (main.py:852-860) — one GPU kernel
        combined_embedding = blend(image_embedding[None], text_embedding[None], weight_image)[0]
        return search_similar(embedding=combined_embedding, limit=limit, filters=filters, min_similarity=min_similarity, n_probe=n_probe,
                              distinct_similarity=distinct_similarity, within_ids=within_ids, where=where, after=after, group_by=group_by)
    except Exception as e:
        logger.error(f"Error in multimodal search: {e}")
        return [] if after is None else _no_page()


def search_multimodal_batch(image_embeddings: np.ndarray, text_embeddings: np.ndarray, weight_image: float = 0.5,
                            limit: int = 10, *, filters: Optional[Sequence[str]] = None,
                            min_similarity: Optional[float] = None, n_probe: Optional[int] = None,
                            distinct_similarity: Optional[float] = None, within_ids: Optional[Sequence[str]] = None,
                            where: Optional[dict] = None, after: Optional[Sequence[Optional[str]]] = None,
                         group_by: Optional[str] = None):
    """BASELINE config 4: a batch of (image, text) embedding pairs, blended and searched in one pass."""
    try:
        return search_similar_batch(blend(image_embeddings, text_embeddings, weight_image), limit, filters=filters,
                                    min_similarity=min_similarity, n_probe=n_probe, distinct_similarity=distinct_similarity,
                                    within_ids=within_ids, where=where, after=after, group_by=group_by)
    except Exception as e:
        logger.error(f"Error in multimodal search: {e}")
        return []


def find_near_duplicates(min_similarity: float = 0.95, limit: Optional[int] = None) -> List[tuple]:
    """Every pair of stored images whose similarity (1 - d / 2) reaches min_similarity -> [(id_a, id_b, similarity_score)],
    each pair once, id_a the earlier upload, ordered by (id_a's upload order, similarity descending). The reference's
    "Duplicate Detection" (README.md:21) is an exact perceptual hash (main.py:628-640): a re-encoded or resized copy passes it.
    limit: at most that many pairs. An image with more than 64 later partners reports its 64 nearest."""
    try:
        col = _collection()
        pairs = col.near_duplicates(float(utils.max_distance_for_similarity(min_similarity)))
        out = [(a, b, 1 - (float(d) / 2)) for a, b, d in pairs]
        return out if limit is None else out[:max(int(limit), 0)]
    except Exception as e:
        logger.error(f"Error searching for near duplicates: {e}")
        return []


def apply_text_filter(filter_query: str, min_similarity: float) -> int:
    """A filter named `filter_query` answered by CLIP itself: every stored image whose similarity (1 - d / 2) to the text's
    embedding reaches min_similarity gets "yes", every other "no" -> the number of "yes" images. The CLIP stand-in for the
    reference's add_filter -> process_filter_on_all_images (main.py:939-1056), whose answers come from a yes/no vision model;
    the searches' `filters=[filter_query]` then work on it as on any stored answer. One pass over the index
    (FlatCollection.add_similarity_filter). Raises what the encoder or the collection raise (a filter half applied is not
    an empty result)."""
    model, processor = utils.load_clip_model()
    embedding = utils.generate_clip_embedding(text=filter_query, model=model, processor=processor)["text"][0]
    return _collection().add_similarity_filter(filter_query, np.asarray(embedding, dtype=np.float32),
                                               float(utils.max_distance_for_similarity(min_similarity)))


def apply_image_filter(image, name: str, min_similarity: float) -> int:
    """apply_text_filter with an example image as the probe: "yes" under `name` for every stored image at least min_similarity
    similar to `image` -> the number of "yes" images."""
    model, processor = utils.load_clip_model()
    embedding = utils.generate_clip_embedding(image=image, model=model, processor=processor)["image"][0]
    return _collection().add_similarity_filter(name, np.asarray(embedding, dtype=np.float32),
                                               float(utils.max_distance_for_similarity(min_similarity)))


def build_search_partition(n_cells: int, iters: int = 10) -> dict:
    """Partition the collection into n_cells k-means cells so that the searches' n_probe has something to probe
    (FlatCollection.build_partition) -> its info dict. Raises what the collection raises."""
    return _collection().build_partition(int(n_cells), iters=int(iters))


def _near_duplicate_of(col, embedding, near_duplicate_similarity):
    """metadata of the nearest stored image within near_duplicate_similarity of `embedding`, or None"""
    hit = col.query(query_embeddings=[embedding], n_results=1, include=["metadatas"],
                    max_distance=float(utils.max_distance_for_similarity(near_duplicate_similarity)))
    if hit["ids"] and hit["ids"][0]:
        return hit["metadatas"][0][0] or {"id": hit["ids"][0][0]}
    return None


def process_image(image, image_id: str, metadata: Optional[Dict[str, Any]] = None, document: str = "",
                  near_duplicate_similarity: Optional[float] = None):
    """The embedding + collection.add portion of process_image (main.py:631-640,685-687,733-744): returns
    (metadata, True) when stored, (existing_metadata, False) for a duplicate id (the caller answers 409).
    Hashing, captioning, background removal and file writes are outside the hot path; the caller supplies the id.
    near_duplicate_similarity: an upload whose embedding has a stored image within that similarity is not stored either:
    (that image's metadata, False) — the same 409 (a re-encoded, resized or lightly cropped copy gets a new hash id)."""
    col = _collection()
    existing = col.get(ids=[image_id], include=["metadatas"])
    if existing and existing["ids"]:
        return existing["metadatas"][0], False
    model, processor = utils.load_clip_model()
    embedding_result = utils.generate_clip_embedding(image, model=model, processor=processor)
    embedding = embedding_result["image"][0].tolist()
    if near_duplicate_similarity is not None:
        twin = _near_duplicate_of(col, embedding, near_duplicate_similarity)
        if twin is not None:
            return twin, False
    metadata = dict(metadata or {})
    metadata.setdefault("id", image_id)
    try:
        col.add(ids=[image_id], embeddings=[embedding], metadatas=[metadata], documents=[document])
    except DuplicateIDError:
        # a concurrent upload of the same image won the race between the check above and this add: same answer as the
        # check would have given (the caller's 409), not a 500
        existing = col.get(ids=[image_id], include=["metadatas"])
        return (existing["metadatas"][0] if existing["ids"] else metadata), False
    return metadata, True


def process_images(images: Sequence, image_ids: Sequence[str], metadatas: Optional[Sequence[dict]] = None,
                   documents: Optional[Sequence[str]] = None, near_duplicate_similarity: Optional[float] = None) -> int:
    """Batched ingest: one encoder pass for all new images, one collection.add. near_duplicate_similarity: images with a stored
    image within that similarity are skipped, as process_image skips them (checked against the collection as it stands before
    the batch, and against the batch's earlier images)."""
    col = _collection()
    have = set(col.get(ids=list(image_ids), include=[])["ids"])
    todo = [i for i, iid in enumerate(image_ids) if iid not in have]
    if not todo:
        return 0
    emb = utils.generate_clip_embeddings(images=[images[i] for i in todo])["image"]
    if near_duplicate_similarity is not None:
        n = 0
        for j, i in enumerate(todo):   # one by one: an image may be the near duplicate of an earlier one of the batch
            if _near_duplicate_of(col, np.asarray(emb[j]).tolist(), near_duplicate_similarity) is None:
                col.add(ids=[image_ids[i]], embeddings=[np.asarray(emb[j]).tolist()],
                        metadatas=[dict((metadatas[i] if metadatas else None) or {"id": image_ids[i]})],
                        documents=[(documents[i] if documents else "")])
                n += 1
        return n
    metas = [dict((metadatas[i] if metadatas else None) or {"id": image_ids[i]}) for i in todo]
    docs = [(documents[i] if documents else "") for i in todo]
    col.add(ids=[image_ids[i] for i in todo], embeddings=emb, metadatas=metas, documents=docs)
    return len(todo)


def classify_collection(prompts: Sequence[str]) -> List[tuple]:
    """Zero-shot classification of the whole collection: which of the text prompts does each stored image match best? ->
    [(image_id, prompt_index, similarity_score)] in upload order, similarity = 1 - d / 2 as everywhere here; an image without a
    direction gets prompt index -1 and similarity None. The prompts are encoded with the text tower and ONE assign call decides
    every image (FlatCollection.assign; ties go to the earlier prompt). Raises what the encoder or the collection raise."""
    prompts = list(prompts)
    if not prompts:
        raise ValueError("classify_collection takes at least one prompt")
    model, processor = utils.load_clip_model()
    emb = np.stack([np.asarray(utils.generate_clip_embedding(text=p, model=model, processor=processor)["text"][0], dtype=np.float32)
                    for p in prompts])
    ids, assign, dist, _sizes = _collection().assign(emb)
    return [(i, int(a), (1 - (float(d) / 2)) if a >= 0 else None) for i, a, d in zip(ids, assign.tolist(), dist.tolist())]


def cluster_collection(n_clusters: int, iters: int = 10) -> tuple:
    """Group the stored images into n_clusters by spherical k-means on their embeddings ("albums", browse by cluster) ->
    ({image_id: cluster}, sizes): cluster -1 for an image without a direction, sizes[c] the images of cluster c. Deterministic
    (FlatIndex.kmeans)."""
    out = _collection().cluster(int(n_clusters), iters=int(iters))
    return dict(zip(out["ids"], (int(a) for a in np.asarray(out["assign"]).tolist()))), [int(v) for v in np.asarray(out["sizes"]).tolist()]
