// Second stage of the field backward's weight-gradient reduction, as a body that more than one kernel can carry: the stand-alone
// dw_finalize_kernel (mlp.hip) and the table backward's accumulate with rider workgroups (gridencoder.hip, pm_accumulate_both_dw_kernel).
// One body, so the order of the additions -- sixteen interleaved slices per element, then slice 0..15 -- is the same wherever it runs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kDwOff[8] = {0, 608, 640, 2880, 6976, 7360, 7552, 7648};      // sigma0 sigma1 color0 color1 color2 spec0 spec1
constexpr int kDwTotal = 7648;
constexpr uint32_t kDwSumBlocks = (kDwTotal + 63) / 64;                    // workgroups of 1024 threads: 64 elements x 16 slices each
struct DwOut { float* dw[7]; };

// `block` = which 64 elements (0 .. kDwSumBlocks), `sm` = 4 KB of the workgroup's LDS; 1024 threads, all of them arrive (one barrier).
__device__ __forceinline__ void dw_sum_body(float (*sm)[64], uint32_t block, const float* __restrict__ part, uint32_t n_rows, const DwOut& o, uint32_t mask,
                                            float* found_inf) {
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int e = block * 64 + lane;
    int mat = 0;
#pragma unroll
    for (int i = 1; i < 7; ++i) mat += e >= kDwOff[i] ? 1 : 0;
    const bool live = e < kDwTotal && ((mask >> mat) & 1u);
    float acc = 0.f;
    if (live) {
        // rows slice, slice + 16, ...: <= 16 per thread for 256 workgroups, all loads of a thread in flight together
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t w = (uint32_t)slice + 16u * i;
            v[i] = w < n_rows ? part[(size_t)w * kDwTotal + e] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) acc += v[i];
        for (uint32_t w = (uint32_t)slice + 256u; w < n_rows; w += 16u) acc += part[(size_t)w * kDwTotal + e];     // larger grids (not used today)
    }
    sm[slice][lane] = acc;
    __syncthreads();
    if (slice == 0 && live) {
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) v += sm[i][lane];
        if (v != 0.f) {
            o.dw[mat][e - kDwOff[mat]] += v;
            if (!(fabsf(v) <= 3.0e38f) && found_inf) *found_inf = 1.0f;
        }
    }
}
