// Test mode (nerf2mesh_amd/camera_path.py): the reference renders a trajectory of cameras that are not in the set (type='test',
// nerf/provider.py:168-184, nerf/colmap_provider.py:346-402) and writes every frame as 8-bit RGB and normalised 8-bit depth
// (Trainer.test, nerf/utils.py:953-1008).  Two entry points: the rays of a camera without images, and a rendered frame as those bytes.
// Compiled with -ffp-contract=off like the rest: every operation below is one fp32 rounding.
#include "n2m_common.hpp"

namespace {

// capture_view_kernel of csrc/capture.hip without the image bank: the same operations in the same order, so the same bits.  Output pixel
// (y, x) of the h x w grid is source pixel (y s, x s); dirs (optional) is safe_normalize(d) repeated ssaa x ssaa times.
__global__ void __launch_bounds__(256)
path_view_kernel(const float* __restrict__ pose /*[4,4]*/, uint32_t h, uint32_t w, uint32_t s, float fx, float fy, float cx, float cy,
                 float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ dirs, uint32_t ssaa) {
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n >= h * w) return;
    const uint32_t y = n / w, x = n % w;
    const float i = (float)(x * s) + 0.5f, j = (float)(y * s) + 0.5f;
    const float d0 = (i - cx) / fx, d1 = -(j - cy) / fy, d2 = -1.0f;
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d[k] = (d0 * pose[4 * k] + d1 * pose[4 * k + 1]) + d2 * pose[4 * k + 2];
        rays_d[(size_t)n * 3 + k] = d[k];
        rays_o[(size_t)n * 3 + k] = pose[4 * k + 3];
    }
    if (dirs) {
        const float len = sqrtf(fmaxf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], 1e-20f));
        const float u0 = d[0] / len, u1 = d[1] / len, u2 = d[2] / len;
        const size_t ws = (size_t)w * ssaa;
        for (uint32_t a = 0; a < ssaa; ++a)
            for (uint32_t b = 0; b < ssaa; ++b) {
                float* __restrict__ q = dirs + (((size_t)y * ssaa + a) * ws + ((size_t)x * ssaa + b)) * 3;
                q[0] = u0; q[1] = u1; q[2] = u2;
            }
    }
}

// (min, max) over the workgroup's 256 threads; valid in thread 0.  All lanes take part (callers hand the identities +FLT_MAX / -FLT_MAX
// for a thread without data).
__device__ __forceinline__ void block_min_max(float& lo, float& hi, float (&sh)[2][4]) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, m));
        hi = fmaxf(hi, __shfl_xor(hi, m));
    }
    if ((threadIdx.x & 63u) == 0) { sh[0][threadIdx.x >> 6] = lo; sh[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
    lo = fminf(fminf(sh[0][0], sh[0][1]), fminf(sh[0][2], sh[0][3]));
    hi = fmaxf(fmaxf(sh[1][0], sh[1][1]), fmaxf(sh[1][2], sh[1][3]));
}

// partials[b] = (min, max) of the elements workgroup b strides over.  Launched with gridDim.x <= ceil(n / 256), so every workgroup has data.
__global__ void __launch_bounds__(256) frame_min_max_kernel(const float* __restrict__ depth, uint32_t n, float* __restrict__ partials) {
    __shared__ float sh[2][4];
    float lo = FLT_MAX, hi = -FLT_MAX;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const float d = depth[i];
        lo = fminf(lo, d);
        hi = fmaxf(hi, d);
    }
    block_min_max(lo, hi, sh);
    if (threadIdx.x == 0) { partials[2 * blockIdx.x] = lo; partials[2 * blockIdx.x + 1] = hi; }
}

constexpr uint32_t PACK_PER_THREAD = 8;      // a workgroup packs 256 * 8 consecutive values, value k * 256 + thread of them per round

// The 4 n values of a frame as one range: [0, 3 n) the image's channels, [3 n, 4 n) the depth.
__global__ void __launch_bounds__(256)
frame_pack_kernel(const float* __restrict__ image, const float* __restrict__ depth, uint32_t n, int linear, const float* __restrict__ partials,
                  uint32_t n_partials, uint8_t* __restrict__ rgb_out, uint8_t* __restrict__ depth_out) {
    __shared__ float sh[2][4];
    float lo = FLT_MAX, hi = -FLT_MAX;
    if (threadIdx.x < n_partials) { lo = partials[2 * threadIdx.x]; hi = partials[2 * threadIdx.x + 1]; }      // n_partials <= 256
    block_min_max(lo, hi, sh);
    const float den = (hi - lo) + 1e-6f;
    const uint64_t n3 = (uint64_t)n * 3, total = (uint64_t)n * 4;
    const uint64_t base = (uint64_t)blockIdx.x * (256 * PACK_PER_THREAD) + threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < PACK_PER_THREAD; ++k) {
        const uint64_t i = base + (uint64_t)k * 256;
        if (i >= total) break;
        if (i < n3) {
            float x = n2m_clampf(image[i], 0.0f, 1.0f);
            if (linear) x = n2m_clampf(x < 0.0031308f ? 12.92f * x : 1.055f * powf(x, 0.41666f) - 0.055f, 0.0f, 1.0f);
            rgb_out[i] = (uint8_t)(uint32_t)(x * 255.0f);
        } else {
            const float d = depth[i - n3];
            depth_out[i - n3] = (uint8_t)(uint32_t)(((d - lo) / den) * 255.0f);
        }
    }
}

}  // namespace

extern "C" int n2m_path_view(const float* poses, uint32_t F, uint32_t frame, uint32_t H, uint32_t W, uint32_t stride, float fx, float fy, float cx,
                             float cy, float* rays_o, float* rays_d, float* dirs, uint32_t ssaa, void* stream) {
    N2M_NOTNULL(poses); N2M_NOTNULL(rays_o); N2M_NOTNULL(rays_d);
    N2M_REQUIRE(frame < F && stride >= 1 && H >= 1 && W >= 1 && (uint64_t)H * W < (1ull << 24), N2M_EINVAL,
                "path_view: need frame < F, stride >= 1 and 1 <= H*W < 2^24");
    N2M_REQUIRE(dirs == nullptr || (ssaa >= 1 && ssaa <= 8), N2M_EINVAL, "path_view: ssaa must be 1..8 when directions are asked for");
    const uint32_t h = H / stride, w = W / stride;
    if (h == 0 || w == 0) return 0;
    path_view_kernel<<<n2m_ceil_div((uint64_t)h * w, 256), 256, 0, (hipStream_t)stream>>>(poses + (size_t)frame * 16, h, w, stride, fx, fy, cx, cy,
                                                                                          rays_o, rays_d, dirs, ssaa);
    N2M_CHECK_LAUNCH();
    return 0;
}

extern "C" int n2m_frame_pack(const float* image, const float* depth, uint32_t n, int linear, uint8_t* rgb_out, uint8_t* depth_out, float* partials,
                              void* stream) {
    N2M_NOTNULL(image); N2M_NOTNULL(depth); N2M_NOTNULL(rgb_out); N2M_NOTNULL(depth_out); N2M_NOTNULL(partials);
    if (n == 0) return 0;
    const uint32_t n_partials = n2m_ceil_div(n, 256) < N2M_FRAME_PACK_PARTIALS ? n2m_ceil_div(n, 256) : N2M_FRAME_PACK_PARTIALS;
    frame_min_max_kernel<<<n_partials, 256, 0, (hipStream_t)stream>>>(depth, n, partials);
    N2M_CHECK_LAUNCH();
    frame_pack_kernel<<<n2m_ceil_div((uint64_t)n * 4, 256 * PACK_PER_THREAD), 256, 0, (hipStream_t)stream>>>(image, depth, n, linear, partials,
                                                                                                           n_partials, rgb_out, depth_out);
    N2M_CHECK_LAUNCH();
    return 0;
}
