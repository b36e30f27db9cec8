// TSDF fusion of per-view depth maps into a truncated signed distance volume -- n2m_tsdf_integrate of include/n2m_hip.h, DESIGN 4.32.
// Not a reference operator: nerf2mesh always thresholds the density lattice (nerf/renderer.py:472-546).
//
// Volume: tsdf, weight [R0,R1,R2] fp32, indexed [x,y,z], z contiguous (marching_cubes' layout).  Lattice point (a,b,c) sits at
//     x_k = lo_k + (float)index_k * step_k,      step_k = (hi_k - lo_k) / (float)(R_k - 1)  (formed once on the host, in fp32),
// a multiply, then an add.  A camera row is 16 floats: R[0..8] the camera-to-world rotation, row-major (R[3 j + k] = row j, column k), the
// centre c[0..2], fx, fy, cx, cy.  The camera looks down its -z axis, y up; pixel (row j, column i) has its centre at (i + 0.5, j + 0.5)
// (capture.rays_from_pixels).  Per lattice point, views v = 0 .. n-1 in this order, every operation one correctly rounded fp32 operation
// (-ffp-contract=off: no FMA), sums associated left to right as written:
//     d   = x - c                                                   (per component)
//     p_k = (R[k] * d_0 + R[3 + k] * d_1) + R[6 + k] * d_2          (p = R^T d: the point in camera axes)
//     zc  = -p_2                                                    skip unless zc > min_depth
//     col = (fx * p_0) / zc + cx,   row = cy - (fy * p_1) / zc      skip unless 0 <= col < W and 0 <= row < H
//     i = floor(col), j = floor(row),  dm = depth[v, j, i]          skip unless dm > 0   (0, negatives and NaN: no information)
//     sdf = dm - zc                                                 skip if sdf < -trunc (+inf is a depth: the ray stops at nothing)
//     s   = min(1, sdf / trunc)
//     tsdf = (tsdf * w + s) / (w + 1),   w = min(w + 1, w_max)
//
// Mapping: voxel-stationary.  One thread owns one lattice point (consecutive lanes = consecutive z, so a wave reads and writes 256
// contiguous bytes of each volume), loads (tsdf, w) once, walks all n views with the state in registers and stores once: the 8 B per voxel
// move once per CALL, not once per view.  The camera row is the same for every lane: its address depends on the loop counter alone, so the
// 16 floats arrive through uniform loads into scalar registers (no LDS, no per-lane traffic).  The depth reads are gathers -- neighbouring
// z lanes project to neighbouring pixels of a 4 H W-byte map, L2 / Infinity Cache traffic.  No atomics, no communication between threads,
// plain vector stores; each voxel's running average is sequential in v, so the result is the same bits on every run and does not depend on
// how the views are split over calls.
#include "n2m_common.hpp"

namespace {

struct TsdfGrid {
    uint32_t R1, R2, total;
    float lo[3], step[3];
};

// One observation: true and s when view `cam` / `depth` says something about the point x.
__device__ __forceinline__ bool tsdf_observe(const float* __restrict__ cam, const float* __restrict__ depth, uint32_t H, uint32_t W,
                                             float x0, float x1, float x2, float trunc, float min_depth, float& s) {
    const float d0 = x0 - cam[9], d1 = x1 - cam[10], d2 = x2 - cam[11];
    const float p0 = (cam[0] * d0 + cam[3] * d1) + cam[6] * d2;
    const float p1 = (cam[1] * d0 + cam[4] * d1) + cam[7] * d2;
    const float p2 = (cam[2] * d0 + cam[5] * d1) + cam[8] * d2;
    const float zc = -p2;
    if (!(zc > min_depth)) return false;
    const float col = (cam[12] * p0) / zc + cam[14];
    const float row = cam[15] - (cam[13] * p1) / zc;
    if (!(col >= 0.f && col < (float)W && row >= 0.f && row < (float)H)) return false;      // NaN fails as well
    const uint32_t i = (uint32_t)col, j = (uint32_t)row;                                      // floor: both are >= 0 and below 2^24
    const float dm = depth[(size_t)j * W + i];
    if (!(dm > 0.f)) return false;
    const float sdf = dm - zc;
    if (sdf < -trunc) return false;
    s = fminf(1.0f, sdf / trunc);
    return true;
}

__global__ void __launch_bounds__(256)
tsdf_integrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight, TsdfGrid g, const float* __restrict__ cams,
                      const float* __restrict__ depth, uint32_t n, uint32_t H, uint32_t W, float trunc, float min_depth, float w_max) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (gid >= (uint64_t)g.total) return;
    const uint32_t idx = (uint32_t)gid;
    const uint32_t c = idx % g.R2, ab = idx / g.R2, b = ab % g.R1, a = ab / g.R1;
    const float x0 = g.lo[0] + (float)a * g.step[0], x1 = g.lo[1] + (float)b * g.step[1], x2 = g.lo[2] + (float)c * g.step[2];
    float t = tsdf[idx], w = weight[idx];
    const size_t map = (size_t)H * W;
#pragma unroll 4
    for (uint32_t v = 0; v < n; ++v) {
        float s = 0.f;
        if (tsdf_observe(cams + 16 * (size_t)v, depth + map * v, H, W, x0, x1, x2, trunc, min_depth, s)) {
            t = (t * w + s) / (w + 1.0f);
            w = fminf(w + 1.0f, w_max);
        }
    }
    tsdf[idx] = t;
    weight[idx] = w;
}

}  // namespace

extern "C" int n2m_tsdf_integrate(float* tsdf, float* weight, uint32_t R0, uint32_t R1, uint32_t R2, const float* lo_host, const float* hi_host,
                                  const float* cams, const float* depth, uint32_t n, uint32_t H, uint32_t W, float trunc, float min_depth,
                                  float w_max, void* stream) {
    N2M_REQUIRE(tsdf && weight && lo_host && hi_host && cams && depth, N2M_ENULL, "tsdf_integrate: NULL tensor");
    N2M_REQUIRE(n > 0 && H > 0 && W > 0, N2M_EINVAL, "tsdf_integrate: empty depth maps (n = %u views of %u x %u pixels; all must be > 0)", n, H, W);
    N2M_REQUIRE(H < (1u << 24) && W < (1u << 24), N2M_EINVAL, "tsdf_integrate: depth maps of %u x %u pixels; each side must be below 2^24", H, W);
    N2M_REQUIRE(R0 >= 2 && R1 >= 2 && R2 >= 2, N2M_EINVAL, "tsdf_integrate: volume %u x %u x %u; every axis needs at least 2 lattice points", R0, R1, R2);
    N2M_REQUIRE(trunc > 0.f, N2M_EINVAL, "tsdf_integrate: trunc must be > 0, got %g", (double)trunc);
    N2M_REQUIRE(w_max >= 1.f, N2M_EINVAL, "tsdf_integrate: w_max must be >= 1, got %g", (double)w_max);
    N2M_REQUIRE(min_depth >= 0.f, N2M_EINVAL, "tsdf_integrate: min_depth must be >= 0, got %g", (double)min_depth);
    for (int k = 0; k < 3; ++k)
        N2M_REQUIRE(hi_host[k] > lo_host[k], N2M_EINVAL, "tsdf_integrate: hi must be above lo on every axis (axis %d: lo %g, hi %g)", k,
                    (double)lo_host[k], (double)hi_host[k]);
    const uint64_t total = (uint64_t)R0 * R1 * R2;
    N2M_REQUIRE(total < (1ull << 32), N2M_EINVAL, "tsdf_integrate: %llu lattice points are beyond 32-bit indexing", (unsigned long long)total);
    TsdfGrid g;
    g.R1 = R1;
    g.R2 = R2;
    g.total = (uint32_t)total;
    const uint32_t R[3] = {R0, R1, R2};
    for (int k = 0; k < 3; ++k) {
        g.lo[k] = lo_host[k];
        g.step[k] = (hi_host[k] - lo_host[k]) / (float)(R[k] - 1u);
    }
    tsdf_integrate_kernel<<<n2m_ceil_div(total, 256), 256, 0, (hipStream_t)stream>>>(tsdf, weight, g, cams, depth, n, H, W, trunc, min_depth, w_max);
    N2M_CHECK_LAUNCH();
    return 0;
}
