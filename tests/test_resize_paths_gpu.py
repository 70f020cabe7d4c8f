"""Every path of the resize / crop kernels (csrc/preprocess_kernels.h), bit for bit against oracle/resize_oracle.py — np.array_equal
on uint8 and int32, no tolerance anywhere. tests/test_resize_paths_cpu.py pins the inputs (tests/resize_cases.py): the oracle is
Pillow at these sizes, the tap counts are as named here, the saturation boards saturate.

test_preprocess_gpu.py stops at 19 taps and at crop sizes that are multiples of 16, so before this file the suite never ran
resize_crop_kernel<0> (the generic tap loop: every image downscaled more than 5.5 x, i.e. every phone photo), never a partial row
or column tile, never more than two 64-row vertical chunks, and saw resize_coeffs_kernel's tables only through the pixels.

  C1 routing at the 11 | 13 and 23 | 25 tap boundaries, one image per launch; C2 workload-shaped generic launches; C3 mixed launches
  (small-tap images inside the generic kernel and inside <24>); C4 partial tiles at S = 98, 266, 8 with a sentinel behind the last
  crop; C5 saturation of the uint8 intermediate image in <24> and <0>; C6 the staged, device-blob and blob-end source routes;
  the vertical-first pass order of images more than 100 times as tall as wide (resize_crop_vfirst_kernel).
  D  resize_coeffs_kernel alone (mmiss_dbg_resize_coeffs): pool and bounds against ro.precompute_coeffs, entry by entry.
Every launch test first asserts, through mmiss_dbg_resize_crop_variant (the function the launcher itself calls), which kernel its
(blob bytes, max ksx) selects. The encoders are TINY-width and carry no weights: the resize needs none."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import resize_cases as rc
from oracle import clip_oracle as co
from oracle import resize_oracle as ro

pytestmark = pytest.mark.gpu

SENT = 0xA5
PATCH = {64: 32, 224: 32, 336: 14, 98: 14, 266: 14, 8: 8}


@pytest.fixture(scope="module")
def env():
    import torch
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib

    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch, _lib, _lib.load()


@pytest.fixture(scope="module")
def encoder(env):
    """encoder(S, max_batch_image): one handle per pair for the whole module."""
    from mmiss_amd.encoder import ClipEncoder, ClipShape

    made = {}

    def get(s, max_batch=8):
        if (s, max_batch) not in made:
            shape = co.TINY if s == co.TINY.v_image else dataclasses.replace(co.TINY, v_patch=PATCH[s], v_image=s)
            made[(s, max_batch)] = ClipEncoder(ClipShape.from_any(shape), max_batch_image=max_batch, max_batch_text=4)
        return made[(s, max_batch)]

    yield get
    for enc in made.values():
        enc.close()


def _ksx(s, hw):
    _, new_w, _, _ = ro.output_geometry(hw[0], hw[1], s)
    return rc.coeffs(hw[1], new_w)[0]


def _pack(images, order=None, gap=0, spare=0):
    """Images laid into one blob in `order` (default: as listed), `gap` unused bytes between neighbours, `spare` behind the last."""
    order = list(range(len(images))) if order is None else order
    offsets = np.zeros(len(images), np.int64)
    parts, pos = [], 0
    for n, i in enumerate(order):
        if n:
            parts.append(np.full(gap, 0xEE, np.uint8))
            pos += gap
        offsets[i] = pos
        parts.append(np.ascontiguousarray(images[i]).reshape(-1))
        pos += images[i].size
    parts.append(np.full(spare, 0xEE, np.uint8))
    hs = np.array([im.shape[0] for im in images], np.int32)
    ws = np.array([im.shape[1] for im in images], np.int32)
    return np.concatenate(parts), offsets, hs, ws


def _call(env, enc, blob, offsets, hs, ws, out):
    """mmiss_resize_crop_rgb on the handle's own stream; blob and out are numpy arrays or torch tensors of the GPU."""
    torch, _lib, lib = env
    torch.cuda.synchronize()        # the handle's stream is not ordered behind torch's
    with enc._call_lock:
        _lib.check(lib.mmiss_encoder_set_stream(enc._h, None, 1))
        nbytes = int(blob.numel() if hasattr(blob, "numel") else blob.size)
        _lib.check(lib.mmiss_resize_crop_rgb(enc._h, _lib.ptr(blob), nbytes, _lib.ptr(offsets), _lib.ptr(hs), _lib.ptr(ws),
                                             len(offsets), _lib.ptr(out)))
    torch.cuda.synchronize()


def _assert_variant(env, blob_bytes, images_ksx, want):
    got = env[2].mmiss_dbg_resize_crop_variant(int(blob_bytes), int(max(images_ksx)))
    assert got == want, f"blob of {blob_bytes} bytes, taps {images_ksx}: kernel <{got}>, this test is about <{want}>"


def _assert_crops(got, wants, what):
    assert got.dtype == np.uint8 and got.shape[0] == len(wants)
    for i, want in enumerate(wants):
        if not np.array_equal(got[i], want):
            bad = np.argwhere((got[i] != want).any(-1))
            raise AssertionError(f"{what}, image {i}: {len(bad)} pixels differ, first at (row, col) {bad[0].tolist()}, "
                                 f"largest difference {np.abs(got[i].astype(int) - want).max()}")


# ---------------------------------------------------------------------------------------------- the launcher's choice
def test_kernel_choice(env):
    v = env[2].mmiss_dbg_resize_crop_variant
    big = 1 << 20
    assert [v(big, k) for k in (5, 11, 12)] == [12, 12, 12]
    assert [v(big, k) for k in (13, 23, 24)] == [24, 24, 24]
    assert [v(big, k) for k in (25, 55, 4095)] == [0, 0, 0]
    assert [v(4, k) for k in (5, 13, 25)] == [12, 24, 0]            # 4 bytes are enough for one 4-byte load
    for nbytes in (0, 3):
        assert [v(nbytes, k) for k in (5, 11, 12, 13, 23, 24, 25, 55, 4095)] == [0] * 9
    assert v(1 << 40, 12) == 12 and v(1 << 40, 25) == 0             # the byte count is 64-bit


# ---------------------------------------------------------------------------------------------- C1
@pytest.mark.parametrize("seed", [2, 3], ids=["noise", "ramps"])
@pytest.mark.parametrize("hw,taps,variant", rc.ROUTING, ids=lambda v: str(v).replace(" ", ""))
def test_routing_boundaries(env, encoder, hw, taps, variant, seed):
    assert _ksx(64, hw) == taps[0]
    _assert_variant(env, hw[0] * hw[1] * 3, [taps[0]], variant)
    got = encoder(64).resize_crop_rgb([rc.img(hw[0], hw[1], seed)])
    _assert_crops(got, [rc.want_crop(64, hw, seed)], f"{hw} alone in <{variant}>")


# ---------------------------------------------------------------------------------------------- C2
@pytest.mark.parametrize("s,hw,taps", rc.WORKLOAD, ids=lambda v: str(v).replace(" ", ""))
def test_workload_shaped_generic(env, encoder, s, hw, taps):
    assert _ksx(s, hw) == taps[0]
    _assert_variant(env, hw[0] * hw[1] * 3, [taps[0]], 0)
    got = encoder(s).resize_crop_rgb([rc.img(hw[0], hw[1], 2)])
    _assert_crops(got, [rc.want_crop(s, hw, 2)], f"{hw} at {s}")


# ---------------------------------------------------------------------------------------------- C3
def _mixed():
    """The five images of the mixed launch (noise and ramps alternate) and their oracle crops."""
    imgs = [rc.img(h, w, 10 + i) for i, (h, w) in enumerate(rc.MIXED)]
    return imgs, [rc.want_crop(64, hw, 10 + i) for i, hw in enumerate(rc.MIXED)]


def test_mixed_launches(env, encoder):
    imgs, wants = _mixed()
    assert [_ksx(64, hw) for hw in rc.MIXED] == rc.MIXED_KSX
    total = sum(im.size for im in imgs)
    enc = encoder(64)
    # all five in one launch: the 5-, 11- and 13-tap images run in the generic kernel
    _assert_variant(env, total, rc.MIXED_KSX, 0)
    _assert_crops(enc.resize_crop_rgb(imgs), wants, "5 images in <0>")
    # reversed: another image ends the blob, every image sits at another offset
    _assert_crops(enc.resize_crop_rgb(imgs[::-1]), wants[::-1], "5 images reversed in <0>")
    # without the 25- and 59-tap images: 5 and 11 taps in <24>, whose taps past xcnt re-read the last pixel with weight 0
    _assert_variant(env, sum(im.size for im in imgs[:3]), rc.MIXED_KSX[:3], 24)
    _assert_crops(enc.resize_crop_rgb(imgs[:3]), wants[:3], "3 images in <24>")
    _assert_crops(enc.resize_crop_rgb(imgs[2::-1]), wants[2::-1], "3 images reversed in <24>")
    # and the two smallest in <12>
    _assert_variant(env, sum(im.size for im in imgs[:2]), rc.MIXED_KSX[:2], 12)
    _assert_crops(enc.resize_crop_rgb(imgs[1::-1]), wants[1::-1], "2 images reversed in <12>")


# ---------------------------------------------------------------------------------------------- C4
@pytest.mark.parametrize("s", sorted(rc.TILE_EDGES))
def test_partial_tiles_and_nothing_behind_the_last_crop(env, encoder, s):
    """S % 16 != 0 and S % 256 != 0: the guards r0 + r < S, the rl clamp, dead columns. Every image alone (its own kernel variant)
    and all in one launch (generic), into a device buffer one crop longer than needed that must keep its sentinel."""
    torch = env[0]
    enc = encoder(s)
    sizes = rc.TILE_EDGES[s][1]
    imgs = [rc.img(hw[0], hw[1], 20 + i) for i, (hw, _) in enumerate(sizes)]
    wants = [rc.want_crop(s, hw, 20 + i) for i, (hw, _) in enumerate(sizes)]
    crop = s * s * 3
    launches = [[i] for i in range(len(imgs))] + [list(range(len(imgs)))]
    for ids in launches:
        sub = [imgs[i] for i in ids]
        ks = [sizes[i][1] for i in ids]
        assert ks == [_ksx(s, sizes[i][0]) for i in ids]
        nbytes = sum(im.size for im in sub)
        _assert_variant(env, nbytes, ks, 12 if max(ks) <= 12 else 24 if max(ks) <= 24 else 0)
        out = torch.full(((len(sub) + 1) * crop,), SENT, dtype=torch.uint8, device="cuda")
        _call(env, enc, *_pack(sub), out)
        got = out.cpu().numpy()
        _assert_crops(got[:len(sub) * crop].reshape(len(sub), s, s, 3), [wants[i] for i in ids], f"S = {s}, images {ids}")
        assert (got[len(sub) * crop:] == SENT).all(), f"S = {s}, images {ids}: bytes behind the last crop were written"


# ---------------------------------------------------------------------------------------------- C5
@pytest.mark.parametrize("hw,b,taps,variant", rc.SATURATION, ids=lambda v: str(v).replace(" ", ""))
def test_saturation_at_many_taps(env, encoder, hw, b, taps, variant):
    """The horizontal sums of these boards leave [0, 255] thousands of times (counted in test_resize_paths_cpu.py): the clip of
    the uint8 intermediate image engages in <24> and in the generic kernel."""
    rgb = rc.checker(hw[0], hw[1], b)
    want = ro.resize_crop_u8(rgb, 64)
    assert want.min() == 0 and want.max() == 255
    assert _ksx(64, hw) == taps
    _assert_variant(env, rgb.size, [taps], variant)
    _assert_crops(encoder(64).resize_crop_rgb([rgb]), [want], f"checkerboard {hw} b = {b} in <{variant}>")


# ---------------------------------------------------------------------------------------------- pass order
def test_pass_order_of_very_tall_images(env, encoder):
    """Found by this file's CPU half: Image.resize runs the vertical pass first when H > 100 W and the height shrinks
    (ro.vertical_first), and the uint8 intermediate image makes that a different result. resize_crop_vfirst_kernel rewrites those
    crops; the images next to the rule (H = 100 W; as tall but upscaled) keep the horizontal-first order. Each alone (<12>; the
    S = 8 one generic), then one launch that mixes both orders, listed both ways."""
    by_s = {}
    for s, hw, ksx, vfirst in rc.PASS_ORDER:
        assert _ksx(s, hw) == ksx and ro.vertical_first(hw[0], hw[1], ro.output_geometry(hw[0], hw[1], s)[0]) == vfirst
        by_s.setdefault(s, []).append((hw, ksx))
    for s, cases in by_s.items():
        enc = encoder(s)
        imgs = [rc.img(hw[0], hw[1], 30 + i) for i, (hw, _) in enumerate(cases)]
        wants = [rc.want_crop(s, hw, 30 + i) for i, (hw, _) in enumerate(cases)]
        for i, (hw, ksx) in enumerate(cases):
            _assert_variant(env, imgs[i].size, [ksx], 12 if ksx <= 12 else 0)
            _assert_crops(enc.resize_crop_rgb([imgs[i]]), [wants[i]], f"{hw} at {s} alone")
        _assert_crops(enc.resize_crop_rgb(imgs), wants, f"S = {s}, both orders in one launch")
        _assert_crops(enc.resize_crop_rgb(imgs[::-1]), wants[::-1], f"S = {s}, both orders in one launch, reversed")


# ---------------------------------------------------------------------------------------------- C6
def test_source_route_host_blob_in_three_staged_chunks(env, encoder):
    """max_batch_image = 2 and 5 images of a host blob: chunks (5, 11), (13, 25), (59) taps cross on the copy stream into the
    two staging buffers while the chunk before them is resized; each is a launch of its own, <12>, <0>, <0>."""
    imgs, wants = _mixed()
    for ids, variant in (([0, 1], 12), ([2, 3], 0), ([4], 0)):
        _assert_variant(env, sum(imgs[i].size for i in ids), [rc.MIXED_KSX[i] for i in ids], variant)
    out = np.zeros((5, 64, 64, 3), np.uint8)
    _call(env, encoder(64, 2), *_pack(imgs), out)
    _assert_crops(out, wants, "host blob, 3 chunks")


@pytest.mark.parametrize("spare", [0, 4], ids=["ends_the_blob", "4_spare_bytes"])
@pytest.mark.parametrize("count,max_batch,order", [(5, 2, [3, 0, 4, 2, 1]), (3, 8, [1, 0, 2])],
                         ids=["5_images_chunks_of_2", "3_images_one_launch"])
def test_source_route_device_blob(env, encoder, count, max_batch, order, spare):
    """A torch blob on the GPU, images shuffled with 7 unused bytes between them. Launches see the WHOLE blob's byte count, so the
    image laid last meets the blob's end from inside a register-tap kernel: with spare = 0 its last row takes the byte-assembled
    loads, with 4 spare bytes the 4-byte loads — the same bytes either way. 5 images, chunks of 2: (5, 11) taps in <12>, the
    11-tap image last in the blob. 3 images, one launch in <24>: the 13-tap image last. By value only: nothing here can see a
    read past the end."""
    torch = env[0]
    imgs, wants = _mixed()
    imgs, wants, ks = imgs[:count], wants[:count], rc.MIXED_KSX[:count]
    blob, offsets, hs, ws = _pack(imgs, order=order, gap=7, spare=spare)
    last = order[-1]
    assert offsets[last] + imgs[last].size + spare == blob.size == sum(im.size for im in imgs) + 7 * (count - 1) + spare
    for b0 in range(0, count, max_batch):
        chunk = ks[b0:b0 + max_batch]
        _assert_variant(env, blob.size, chunk, 12 if max(chunk) <= 12 else 24 if max(chunk) <= 24 else 0)
    first_chunk = ks[:max_batch]
    assert last < max_batch and max(first_chunk) <= 24, "the image that ends the blob must run in a register-tap kernel"
    dev = torch.from_numpy(blob).cuda()
    out = np.zeros((count, 64, 64, 3), np.uint8)
    _call(env, encoder(64, max_batch), dev, offsets, hs, ws, out)
    _assert_crops(out, wants, f"device blob, order {order}, {spare} spare bytes")


# ---------------------------------------------------------------------------------------------- D
COEFF_GROUPS = {
    "crop_test_sizes": rc.image_cases(), "power_of_two_ratios": rc.POW2, "thin_edges": rc.THIN, "upscales": rc.UPSCALE,
    "prime_edges": rc.PRIME, "limits": rc.LIMITS, "random_224": rc.random_cases()[:40], "random_64": rc.random_cases()[40:],
}


def test_coefficient_groups_cover_the_sweep():
    assert sorted(set(c for g in COEFF_GROUPS.values() for c in g)) == sorted(rc.coeff_cases())


@pytest.mark.parametrize("group", list(COEFF_GROUPS))
def test_coefficient_tables(env, group):
    """resize_geometry and one resize_coeffs_kernel launch against ro.output_geometry / ro.precompute_coeffs: the geometry field by
    field, bounds over the crop window, every reserved tap of kx [ksx][S] and ky [S][ksy] (the oracle's rows are zero past their
    count, as the kernel's must be), and nothing written behind either table."""
    torch, _lib, lib = env
    pad, sent = 64, -123456789
    for s, (h, w) in COEFF_GROUPS[group]:
        what = f"{h} x {w} -> {s}"
        new_h, new_w, top, left = ro.output_geometry(h, w, s)
        ksx, bx, kkx = rc.coeffs(w, new_w)
        ksy, by, kky = rc.coeffs(h, new_h)
        geo = (C.c_int32 * 6)()
        _lib.check(lib.mmiss_dbg_resize_coeffs(0, None, h, w, s, geo, None, None))
        assert tuple(geo) == (new_h, new_w, top, left, ksx, ksy), what
        n_pool = (ksx + ksy) * s
        pool = torch.full((n_pool + pad,), sent, dtype=torch.int32, device="cuda")
        bounds = torch.full((4 * s + pad,), sent, dtype=torch.int32, device="cuda")
        geo2 = (C.c_int32 * 6)()
        _lib.check(lib.mmiss_dbg_resize_coeffs(0, _lib.current_stream_ptr(), h, w, s, geo2, pool.data_ptr(), bounds.data_ptr()))
        assert tuple(geo2) == tuple(geo), what
        pool, bounds = pool.cpu().numpy(), bounds.cpu().numpy()
        assert (pool[n_pool:] == sent).all() and (bounds[4 * s:] == sent).all(), what
        got_b = bounds[:4 * s].reshape(4, s)
        assert np.array_equal(got_b[0], bx[left:left + s, 0]) and np.array_equal(got_b[1], bx[left:left + s, 1]), what
        assert np.array_equal(got_b[2], by[top:top + s, 0]) and np.array_equal(got_b[3], by[top:top + s, 1]), what
        kx = pool[:ksx * s].reshape(ksx, s)
        ky = pool[ksx * s:n_pool].reshape(s, ksy)
        for name, got, want in (("kx", kx, kkx[left:left + s].T), ("ky", ky, kky[top:top + s])):
            if not np.array_equal(got, want):
                bad = np.argwhere(got != want)
                raise AssertionError(f"{what}: {name} differs at {len(bad)} entries, first {bad[0].tolist()}: "
                                     f"{got[tuple(bad[0])]} against {want[tuple(bad[0])]}")


def test_coefficient_entry_refusals(env):
    torch, _lib, lib = env
    geo = (C.c_int32 * 6)()
    one = torch.zeros(16, dtype=torch.int32, device="cuda")
    assert lib.mmiss_dbg_resize_coeffs(0, None, 8, 8, 8, geo, one.data_ptr(), None) != 0      # one table without the other
    assert lib.mmiss_dbg_resize_coeffs(0, None, 8, 8, 8, None, None, None) != 0
    assert lib.mmiss_dbg_resize_coeffs(0, None, 65536, 65536, 8, geo, one.data_ptr(), one.data_ptr()) != 0   # 32769 taps
