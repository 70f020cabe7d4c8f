// What the resize kernels of preprocess_kernels.h (compiled into api_encoder.hip) and preprocess_vfirst.hip share.
#pragma once
#include "common.h"

struct ResizeDesc {
    int64_t src_off;        // byte offset of the image (tightly packed RGB8, row stride 3*W) inside the source blob
    int32_t H, W;           // source size
    int32_t new_h, new_w;   // resized size (shortest edge = S)
    int32_t top, left;      // centre-crop offsets inside the resized image
    int32_t ksx, ksy;       // taps reserved per output index (Pillow's ksize) on x / y
    int64_t kx_off, ky_off; // int32 offsets into the coefficient pool: kx[tap][S] (tap-major), ky[S][ksy]
};

#define MMISS_RESIZE_PRECISION_BITS 22
#define MMISS_RESIZE_ROWS 16

__device__ __forceinline__ int clip8_fixed(int32_t v) {
    v >>= MMISS_RESIZE_PRECISION_BITS;  // arithmetic shift, as Pillow's clip8
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Pillow's rule for the pass order (Image.resize): vertical first on images more than 100 times as tall as wide whose height shrinks
__host__ __device__ static inline bool resize_vertical_first(int H, int W, int new_h) { return H > W * 100 && new_h < H; }
#define MMISS_RESIZE_VFIRST_MAX_W 655   // H <= 65536 and H > 100 W

// preprocess_vfirst.hip: the crops of the images resize_vertical_first selects, over what resize_crop_kernel wrote for them
void launch_resize_crop_vfirst(hipStream_t st, const uint8_t* src, const ResizeDesc* desc, const int32_t* pool,
                               const int32_t* bounds, uint8_t* dst, int S, int nb);
