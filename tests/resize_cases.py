"""Sizes, images and cached oracle tables shared by test_resize_paths_cpu.py (which pins these inputs: Pillow parity, tap counts,
int32 headroom, saturation) and test_resize_paths_gpu.py (which runs them through the kernels). Not a test module.

A case names the image size (H, W), the crop size S, the oracle's tap counts (ksx, ksy) and, where one image is one launch, the
resize_crop_kernel<KMAX> variant its ksx selects (12 / 24 / 0 = generic)."""
import functools

import numpy as np

from oracle import resize_oracle as ro

# ---------------------------------------------------------------------------------------------- C1: routing boundaries, S = 64
# (H, W), (ksx, ksy), variant of the image alone
ROUTING = [
    ((150, 170), (11, 11), 12),
    ((161, 200), (13, 13), 24),
    ((353, 352), (23, 25), 24),   # y taps above x taps: only ksx routes
    ((352, 353), (25, 23), 0),
    ((900, 1200), (59, 59), 0),   # 14 x 16 source rows per 16-row tile: several 64-row vertical chunks
    ((1, 1), (5, 5), 0),          # a 3-byte blob: the blob_bytes < 4 branch
]
# ---------------------------------------------------------------------------------------------- C2: workload-shaped generic cases
# S, (H, W), (ksx, ksy)
WORKLOAD = [
    (224, (3000, 4000), (55, 55)),
    (224, (1233, 1300), (25, 25)),
    (336, (2000, 1900), (25, 25)),   # two column blocks
]
# ---------------------------------------------------------------------------------------------- C3 / C6: one mixed launch, S = 64
MIXED = [(33, 40), (150, 170), (161, 200), (352, 353), (900, 1200)]
MIXED_KSX = [5, 11, 13, 25, 59]
# ---------------------------------------------------------------------------------------------- C4: partial tiles
# S -> (patch, [((H, W), ksx)]): 98 = 6 * 16 + 2; 266 = 16 * 16 + 10 = 256 + 10; 8 = one partial tile, 248 dead columns.
# Every S holds a 12-, a 24- and a generic-kernel image, so each variant meets each partial tile when an image runs alone.
TILE_EDGES = {
    98: (14, [((300, 260), 13), ((700, 540), 25), ((97, 99), 5)]),
    266: (14, [((300, 280), 7), ((900, 1000), 15), ((1500, 1470), 25)]),
    8: (8, [((100, 90), 47), ((5, 7), 5), ((8, 8), 5), ((30, 28), 15)]),
}
# ---------------------------------------------------------------------------------------------- C5: saturation, S = 64
# (H, W), checker block, ksx, variant
SATURATION = [((230, 250), 5, 17, 24), ((400, 420), 9, 27, 0)]
# ---------------------------------------------------------------------------------------------- pass order (found by this sweep)
# Image.resize runs the vertical pass FIRST when H > 100 W and the height shrinks (ro.vertical_first). S, (H, W), ksx, vertical first?
PASS_ORDER = [
    (64, (7000, 69), 7, True),
    (64, (6901, 69), 7, True),     # the smallest H above 100 W
    (64, (6900, 69), 7, False),    # H = 100 W exactly: horizontal first
    (64, (7000, 60), 5, False),    # as tall, but upscaled: horizontal first
    (8, (9100, 90), 47, True),     # in a launch of the generic kernel
]


def image_cases():
    """Every (S, (H, W)) that sections C1 .. C6 push through the crop kernels, once each."""
    out = [(64, hw) for hw, _, _ in ROUTING]
    out += [(s, hw) for s, hw, _ in WORKLOAD]
    out += [(64, hw) for hw in MIXED]
    out += [(s, hw) for s, (_, sizes) in TILE_EDGES.items() for hw, _ in sizes]
    out += [(64, hw) for hw, _, _, _ in SATURATION]
    out += [(s, hw) for s, hw, _, _ in PASS_ORDER]
    return list(dict.fromkeys(out))


# ---------------------------------------------------------------------------------------------- D: coefficient sweep
POW2 = [(224, (448, 448)), (224, (896, 896)), (224, (1792, 1792)), (224, (3584, 3584)), (224, (448, 3584)),
        (64, (128, 128)), (64, (512, 512)), (64, (512, 128))]                    # centres on exact halves
THIN = [(s, hw) for s in (224, 64) for hw in [(1, 1), (1, 2), (2, 1), (2, 2), (1, 40), (40, 1), (2, 31), (300, 2)]]
UPSCALE = [(224, (3, 500)), (224, (17, 17)), (224, (1, 1)), (64, (17, 17))]
PRIME = [(224, (997, 1009)), (224, (4093, 3001)), (64, (997, 1009))]
LIMITS = [(224, (65536, 65536)), (224, (65536, 300))]                            # 1173 taps; tables of about 1 MB


def random_cases():
    rng = np.random.default_rng(20240611)
    hw = rng.integers(1, 5001, (40, 2))
    return [(s, (int(h), int(w))) for s in (224, 64) for h, w in hw]


def coeff_cases():
    return list(dict.fromkeys(image_cases() + POW2 + THIN + UPSCALE + PRIME + LIMITS + random_cases()))


def headroom_axes():
    """(in, out) axes named for the int32 headroom figure: the widest filter, the narrowest, the largest upscale."""
    return [(4000, 298), (3000, 224), (640, 298), (65536, 224), (1240, 224), (17, 224), (500, 37333)]


# ---------------------------------------------------------------------------------------------- images
def img(h, w, seed):
    """test_preprocess_gpu.py's generator: noise for an even seed, smooth ramps for an odd one."""
    rng = np.random.default_rng(seed)
    if seed % 2:
        yy, xx = np.mgrid[0:h, 0:w]
        return np.stack([(yy * 255 // max(h - 1, 1)), (xx * 255 // max(w - 1, 1)), ((yy * 3 + xx * 5) % 256)], -1).astype(np.uint8)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def checker(h, w, b):
    """Black / white blocks of b pixels, with the channel-inverted copy in G (test_preprocess_gpu.py's saturation image)."""
    yy, xx = np.mgrid[0:h, 0:w]
    chk = (((yy // b + xx // b) % 2) * 255).astype(np.uint8)
    return np.stack([chk, 255 - chk, chk], -1)


# ---------------------------------------------------------------------------------------------- cached oracle
@functools.lru_cache(maxsize=None)
def coeffs(in_size, out_size):
    """ro.precompute_coeffs, once per axis and process (a Python loop over out_size)."""
    return ro.precompute_coeffs(in_size, out_size)


@functools.lru_cache(maxsize=None)
def _crop(s, h, w, seed):
    out = ro.resize_crop_u8(img(h, w, seed), s)
    out.setflags(write=False)
    return out


def want_crop(s, hw, seed):
    """The oracle's crop of img(h, w, seed), computed once and read-only."""
    return _crop(s, hw[0], hw[1], seed)
