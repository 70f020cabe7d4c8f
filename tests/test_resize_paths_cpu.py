"""The inputs of tests/test_resize_paths_gpu.py are what they claim, and oracle/resize_oracle.py is Pillow there (sizes, tap counts
and images in tests/resize_cases.py).

  * oracle == Pillow, bit for bit, at every image the crop kernels are run on and at the named sizes of the coefficient sweep
    (test_resize_oracle_cpu.py stops at 2000 x 1500 and S = 224). The sweep's 65536 x 65536 case is 12.9 GB as an image and its
    80 random cases would cost half a minute as images: their AXES are pinned instead, on 6-pixel strips — Pillow's coefficients
    of an axis depend on (in, out) of that axis alone, and a pass over an axis that keeps its size is the identity in both.
  * the tap counts the GPU tests name are the oracle's, so an edit of a size table cannot move a case off its kernel silently.
  * int32 headroom of both passes, derived from the coefficient rows: 2^21 + 255 * (sum of the positive k) < 2^31, and the negative
    side likewise. Worst figure over the named axes and every axis of the image cases: 1 214 385 512 = 0.565 * 2^31 (printed).
  * the checkerboards of the saturation test do drive the horizontal sums out of [0, 255], > 1000 times each (restated here from
    the oracle's tables: the oracle clips before anything can be counted), and a finer board (b = 4 / b = 7) would not.
  * the library's host geometry (new size, crop offsets, tap counts, the 4096-tap refusal) equals the oracle's on a sweep that
    needs no device: mmiss_dbg_resize_coeffs with null tables."""
import math

import numpy as np
import pytest

import resize_cases as rc
from oracle import clip_oracle as co
from oracle import resize_oracle as ro

Image = pytest.importorskip("PIL.Image")

IMAGES = rc.image_cases() + [c for c in rc.POW2 + rc.THIN + rc.UPSCALE + rc.PRIME + rc.LIMITS if c[1] != (65536, 65536)]
IMAGES = list(dict.fromkeys(IMAGES))


def _geometry(s, hw):
    new_h, new_w, top, left = ro.output_geometry(hw[0], hw[1], s)
    return new_h, new_w, top, left


@pytest.mark.parametrize("s,hw", IMAGES, ids=lambda v: str(v).replace(" ", ""))
def test_oracle_equals_pillow_on_the_images(s, hw):
    for seed in (2, 3):                                   # noise, ramps
        if seed == 3 and hw[0] * hw[1] > 4_000_000:
            continue                                      # (the large images once: Pillow parity does not hinge on the content)
        rgb = rc.img(hw[0], hw[1], seed)
        assert np.array_equal(ro.resize_crop_u8(rgb, s), co.crop_u8(Image.fromarray(rgb), s)), (s, hw, seed)


def test_oracle_equals_pillow_on_the_saturation_boards():
    for hw, b, _, _ in rc.SATURATION:
        rgb = rc.checker(hw[0], hw[1], b)
        assert np.array_equal(ro.resize_crop_u8(rgb, 64), co.crop_u8(Image.fromarray(rgb), 64)), (hw, b)


def test_pass_order_changes_bytes_and_the_oracle_follows_pillow():
    """Image.resize (PIL/Image.py) resamples vertically first when H > 100 W and the height shrinks. This file found it: the oracle,
    horizontal first everywhere until then, was off by one in most pixels of the sweep's 65536 x 300 image. The cases around the
    rule equal Pillow (above, through IMAGES); here: on those the rule selects, the horizontal-first result is a DIFFERENT image,
    so a kernel that ignores the rule cannot pass."""
    for s, hw, _, vfirst in rc.PASS_ORDER:
        rgb = rc.img(hw[0], hw[1], 2)
        new_h, new_w, top, left = _geometry(s, hw)
        assert ro.vertical_first(hw[0], hw[1], new_h) == vfirst
        _, bx, kx = rc.coeffs(hw[1], new_w)
        _, by, ky = rc.coeffs(hw[0], new_h)
        tmp = ro._pass(np.ascontiguousarray(rgb.transpose(1, 0, 2)), bx, kx, left, s).transpose(1, 0, 2)
        hfirst = ro._pass(np.ascontiguousarray(tmp), by, ky, top, s)
        assert np.array_equal(hfirst, ro.resize_crop_u8(rgb, s)) == (not vfirst), (s, hw)


def test_oracle_equals_pillow_on_every_axis_of_the_sweep():
    """One strip per distinct (in, out, first) axis of the coefficient sweep: Pillow resizes [6, in] -> [6, out], the oracle computes
    the crop window's S indices of it. The other axis keeps its size, and Pillow skips that pass."""
    axes = set()
    for s, hw in rc.coeff_cases():
        new_h, new_w, top, left = _geometry(s, hw)
        axes |= {(hw[0], new_h, top, s), (hw[1], new_w, left, s)}
    assert (65536, 224, 0, 224) in axes and len(axes) > 150
    for n_in, n_out, first, s in sorted(axes):
        strip = np.random.default_rng(n_in * 131 + n_out).integers(0, 256, (6, n_in, 3), dtype=np.uint8)
        want = np.asarray(Image.fromarray(strip).resize((n_out, 6), resample=Image.BICUBIC))[:, first:first + s]
        _, bounds, kk = rc.coeffs(n_in, n_out)
        got = ro._pass(np.ascontiguousarray(strip.transpose(1, 0, 2)), bounds, kk, first, s).transpose(1, 0, 2)
        assert np.array_equal(got, want), (n_in, n_out)
    for n_in, n_out in [(4093, 224), (997, 224), (3, 224)]:      # the vertical pass of Pillow takes the same tables
        strip = np.random.default_rng(n_in).integers(0, 256, (n_in, 6, 3), dtype=np.uint8)
        want = np.asarray(Image.fromarray(strip).resize((6, n_out), resample=Image.BICUBIC))
        _, bounds, kk = rc.coeffs(n_in, n_out)
        assert np.array_equal(ro._pass(strip, bounds, kk, 0, n_out), want), (n_in, n_out)


def test_tap_counts_are_as_the_gpu_tests_name_them():
    def taps(s, hw):
        new_h, new_w, _, _ = _geometry(s, hw)
        return rc.coeffs(hw[1], new_w)[0], rc.coeffs(hw[0], new_h)[0]

    def variant(ksx):
        return 12 if ksx <= 12 else 24 if ksx <= 24 else 0

    for hw, k, v in rc.ROUTING:
        assert taps(64, hw) == k, hw
        assert v == (0 if hw == (1, 1) else variant(k[0])), hw          # 1 x 1 alone: a 3-byte blob, generic whatever the taps
    for s, hw, k in rc.WORKLOAD:
        assert taps(s, hw) == k and variant(k[0]) == 0, (s, hw)
    assert [taps(64, hw)[0] for hw in rc.MIXED] == rc.MIXED_KSX == [5, 11, 13, 25, 59]
    for s, (patch, sizes) in rc.TILE_EDGES.items():
        assert s % patch == 0
        assert {variant(k) for _, k in sizes} == {12, 24, 0}, s
        for hw, k in sizes:
            assert taps(s, hw)[0] == k, (s, hw)
    for hw, _, k, v in rc.SATURATION:
        assert taps(64, hw) == (k, k) and variant(k) == v, hw
    for s, hw, k, vfirst in rc.PASS_ORDER:
        assert taps(s, hw)[0] == k and ro.vertical_first(hw[0], hw[1], _geometry(s, hw)[0]) == vfirst, (s, hw)
    assert (98 % 16, 266 % 16, 266 % 256, 8 % 16) == (2, 10, 10, 8)      # the partial tiles the GPU file is after
    assert taps(224, (65536, 65536)) == (1173, 1173)


def _headroom(kk):
    """Largest |2^21 + sum| a pass can reach with these rows and pixels in 0..255: (positive side, negative side)."""
    k = kk.astype(np.int64)
    pos = 255 * np.where(k > 0, k, 0).sum(1).max() + (1 << 21)
    neg = 255 * np.where(k < 0, k, 0).sum(1).min() + (1 << 21)
    return int(pos), int(neg)


def test_int32_headroom_of_both_passes():
    axes = set(rc.headroom_axes())
    for s, hw in rc.image_cases():
        new_h, new_w, _, _ = _geometry(s, hw)
        axes |= {(hw[0], new_h), (hw[1], new_w)}
    worst_pos, worst_neg = 0, 0
    for n_in, n_out in sorted(axes):
        pos, neg = _headroom(rc.coeffs(n_in, n_out)[2])
        assert pos < 2 ** 31 and neg >= -(2 ** 31), (n_in, n_out, pos, neg)
        worst_pos, worst_neg = max(worst_pos, pos), min(worst_neg, neg)
    print(f"int32 headroom: largest positive sum {worst_pos} = {worst_pos / 2 ** 31:.3f} * 2^31, most negative {worst_neg}")


def _horizontal_sums_outside(rgb, s):
    """How many horizontal-pass sums of the crop window's columns, before the clip, leave [0, 255] (all H rows, 3 channels)."""
    h, w, _ = rgb.shape
    _, new_w, _, left = _geometry(s, (h, w))
    _, bounds, kk = rc.coeffs(w, new_w)
    out = 0
    for i in range(left, left + s):
        xmin, n = bounds[i]
        acc = (rgb[:, xmin:xmin + n].astype(np.int64) * kk[i, :n].astype(np.int64)[None, :, None]).sum(1) + (1 << 21)
        v = acc >> 22
        out += int(((v < 0) | (v > 255)).sum())
    return out


def test_saturation_boards_do_saturate():
    counts = {}
    for hw, b, _, _ in rc.SATURATION:
        counts[(hw, b)] = _horizontal_sums_outside(rc.checker(hw[0], hw[1], b), 64)
        assert counts[(hw, b)] > 1000, counts
        crop = ro.resize_crop_u8(rc.checker(hw[0], hw[1], b), 64)
        assert crop.min() == 0 and crop.max() == 255
    print("horizontal sums outside [0, 255]:", counts)
    # and the block size matters: one pixel finer and the filter averages the board away
    assert _horizontal_sums_outside(rc.checker(230, 250, 4), 64) == 0
    assert _horizontal_sums_outside(rc.checker(400, 420, 7), 64) == 0


# ---------------------------------------------------------------------------------------------- the host geometry of the library
def _ksize(in_size, out_size):
    """ro.precompute_coeffs' ksize without its loop over the outputs (pinned against it below)."""
    scale = float(np.float32(in_size) - np.float32(0.0)) / out_size
    return int(math.ceil(2.0 * (scale if scale >= 1.0 else 1.0))) * 2 + 1


def test_library_geometry_sweep():
    """resize_geometry as the library runs it (mmiss_dbg_resize_coeffs with null tables: host arithmetic only, no device) against
    ro.output_geometry and the oracle's ksize: every (H, W) in 1..40 x 1..40, 2000 random pairs up to 65536 and the tap limit's
    neighbours, at S = 8, 64, 224, 336. What needs more than 4096 taps is refused, nothing else is."""
    import ctypes as C

    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib

    lib = _lib.load()
    err_arg, err_unsupported = -1, -5                      # include/mmiss.h
    for s, hw in rc.coeff_cases():
        new_h, new_w, _, _ = _geometry(s, hw)
        assert (_ksize(hw[1], new_w), _ksize(hw[0], new_h)) == (rc.coeffs(hw[1], new_w)[0], rc.coeffs(hw[0], new_h)[0])
    rng = np.random.default_rng(77)
    pairs = [(h, w) for h in range(1, 41) for w in range(1, 41)] + [tuple(int(v) for v in p) for p in rng.integers(1, 65537, (2000, 2))]
    pairs += [(65536, 65536), (65535, 65535), (65472, 65472), (65473, 65536), (1, 65536), (65536, 1), (8192, 8192), (8193, 8193)]
    geo = (C.c_int32 * 6)()
    refused = 0
    for s in (8, 64, 224, 336):
        for h, w in pairs:
            new_h, new_w, top, left = ro.output_geometry(h, w, s)
            ksx, ksy = _ksize(w, new_w), _ksize(h, new_h)
            status = lib.mmiss_dbg_resize_coeffs(0, None, h, w, s, geo, None, None)
            if ksx > 4096 or ksy > 4096:
                assert status == err_unsupported, (h, w, s, ksx, ksy)
                refused += 1
            else:
                assert status == 0 and tuple(geo) == (new_h, new_w, top, left, ksx, ksy), (h, w, s, tuple(geo))
    assert refused > 100                                    # (S = 8: every short edge above 8188; S = 64: 65473 and up)
    assert lib.mmiss_dbg_resize_coeffs(0, None, 65472, 65472, 64, geo, None, None) == 0 and geo[4] == 4093
    assert lib.mmiss_dbg_resize_coeffs(0, None, 65473, 65536, 64, geo, None, None) == err_unsupported
    for h, w, s in ((0, 5, 64), (5, 0, 64), (65537, 5, 64), (5, 65537, 64), (5, 5, 0), (-1, -1, 64)):
        assert lib.mmiss_dbg_resize_coeffs(0, None, h, w, s, geo, None, None) == err_arg, (h, w, s)
