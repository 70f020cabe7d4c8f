"""Radius queries end to end on the MI355X: a FlatCollection on a real index behind mmiss_amd.search (tiny seeded CLIP, real HIP
kernels). search_similar(min_similarity=s) is the cut of the full ranking at s, and an upload one pixel away from a stored image
is refused under near_duplicate_similarity."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture()
def stack():
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection, search, utils
    from mmiss_amd.encoder import ClipEncoder, ClipShape
    from mmiss_amd.preprocess import ClipProcessor
    from oracle import clip_oracle as co

    shape = dataclasses.replace(co.TINY, v_image=224)
    enc = ClipEncoder(ClipShape.from_any(shape), max_batch_image=8, max_batch_text=8)
    enc.load_state_dict(co.init_weights(shape, seed=11))
    utils.set_clip_model(enc, ClipProcessor(ClipShape.from_any(shape), tokenizer=None, max_length=shape.t_ctx))
    col = collection.FlatCollection("radius-e2e")
    search.set_collection(col)
    yield search, col, shape
    utils.set_clip_model(None, None)
    search.set_collection(None)


def _image(seed, touch=False):
    from PIL import Image

    a = np.random.Generator(np.random.Philox(seed)).integers(0, 256, size=(240, 300, 3), dtype=np.uint8)
    if touch:
        a[100, 120, 1] ^= 1
    return Image.fromarray(a)


def test_min_similarity_is_the_cut_of_the_ranking(stack):
    search, col, shape = stack
    rng = np.random.Generator(np.random.Philox(4))
    D = shape.proj_dim
    base = rng.standard_normal((8, D)).astype(np.float32)
    v = np.concatenate([b + s * rng.standard_normal((25, D)).astype(np.float32) for b, s in zip(base, np.linspace(0.05, 1.0, 8))])
    col.add(ids=[f"im{i:03d}" for i in range(v.shape[0])], embeddings=v, metadatas=[{"id": f"im{i:03d}"} for i in range(v.shape[0])])
    full = search.search_similar(base[2], limit=col.count())
    assert len(full) == 200
    sims = [r["similarity_score"] for r in full]
    for s in (0.0, 0.5, sims[30], float(np.nextafter(sims[30], 2.0)), 0.9, 0.99, 1.0):
        got = search.search_similar(base[2], limit=col.count(), min_similarity=s)
        assert got == [r for r in full if r["similarity_score"] >= s], s
    assert 0 < len(search.search_similar(base[2], limit=col.count(), min_similarity=0.9)) < 200
    assert search.search_similar(base[2], limit=7, min_similarity=0.5) == [r for r in full if r["similarity_score"] >= 0.5][:7]
    assert col._index.guard_stats()["radius_queries"] == 9
    pairs = search.find_near_duplicates(min_similarity=0.99)
    assert pairs and all(a < b and s >= 0.99 for a, b, s in pairs)


def test_upload_one_pixel_away_is_refused(stack):
    search, col, shape = stack
    meta, stored = search.process_image(_image(1), "first", {"id": "first", "note": "original"}, near_duplicate_similarity=0.98)
    assert stored
    meta, stored = search.process_image(_image(1, touch=True), "second", {"id": "second"}, near_duplicate_similarity=0.98)
    assert not stored and meta["id"] == "first" and meta["note"] == "original"
    assert col.count() == 1
    # without the argument the same upload is stored, as before (seeded noise images through seeded random towers all embed
    # within 0.98 of each other, so "a different image is still stored" is shown on the CPU, tests/test_radius_layers_cpu.py)
    meta, stored = search.process_image(_image(1, touch=True), "second", {"id": "second"})
    assert stored and col.count() == 2
