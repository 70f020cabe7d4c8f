// The vertical-first order of Pillow's resize (see preprocess_kernels.h), kept out of api_encoder.hip's code object.
#include "preprocess_common.h"

// grid (S, B), block 256: output row blockIdx.x of image blockIdx.y, only for the images resize_vertical_first selects (the others
// return at once: resize_crop_kernel has written them). The block resamples its row vertically over the full width into LDS (uint8,
// Pillow's intermediate image), then horizontally from there; same tables and bounds as resize_crop_kernel. Byte loads only.
__global__ __launch_bounds__(256) void resize_crop_vfirst_kernel(const uint8_t* __restrict__ src,
                                                                 const ResizeDesc* __restrict__ desc,
                                                                 const int32_t* __restrict__ pool,
                                                                 const int32_t* __restrict__ bounds,
                                                                 uint8_t* __restrict__ dst, int S) {
    constexpr int32_t HALF = 1 << (MMISS_RESIZE_PRECISION_BITS - 1);
    __shared__ uint8_t mid[MMISS_RESIZE_VFIRST_MAX_W * 3];
    const int r = blockIdx.x, b = blockIdx.y;
    const ResizeDesc d = desc[b];
    if (!resize_vertical_first(d.H, d.W, d.new_h) || d.W > MMISS_RESIZE_VFIRST_MAX_W) return;  // block-uniform
    const int32_t* bnd = bounds + (size_t)b * 4 * S;
    const int ymin = bnd[2 * S + r], ycnt = bnd[3 * S + r];
    const int32_t* ky = pool + d.ky_off + (int64_t)r * d.ksy;
    const int row_bytes = d.W * 3;
    const uint8_t* p = src + d.src_off + (int64_t)ymin * row_bytes;
    for (int i = threadIdx.x; i < row_bytes; i += 256) {   // byte i of a row = channel i % 3 of pixel i / 3
        int32_t s = HALF;
        for (int y = 0; y < ycnt; ++y) s += (int32_t)p[(int64_t)y * row_bytes + i] * ky[y];
        mid[i] = (uint8_t)clip8_fixed(s);
    }
    __syncthreads();
    for (int col = threadIdx.x; col < S; col += 256) {
        const int xmin = bnd[col], xcnt = bnd[S + col];
        const int32_t* kx = pool + d.kx_off + col;
        const uint8_t* q = mid + xmin * 3;
        int32_t s0 = HALF, s1 = HALF, s2 = HALF;
        for (int x = 0; x < xcnt; ++x) {
            const int32_t k = kx[(int64_t)x * S];
            s0 += (int32_t)q[x * 3] * k;
            s1 += (int32_t)q[x * 3 + 1] * k;
            s2 += (int32_t)q[x * 3 + 2] * k;
        }
        uint8_t* o = dst + (((int64_t)b * S + r) * S + col) * 3;
        o[0] = (uint8_t)clip8_fixed(s0);
        o[1] = (uint8_t)clip8_fixed(s1);
        o[2] = (uint8_t)clip8_fixed(s2);
    }
}

void launch_resize_crop_vfirst(hipStream_t st, const uint8_t* src, const ResizeDesc* desc, const int32_t* pool,
                               const int32_t* bounds, uint8_t* dst, int S, int nb) {
    hipLaunchKernelGGL(resize_crop_vfirst_kernel, dim3(S, nb), dim3(256), 0, st, src, desc, pool, bounds, dst, S);
}
