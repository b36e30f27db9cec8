// Captured image sets (nerf2mesh_amd/capture.py): the reference keeps its training images on the device as uint8 [N,H,W,3|4], divides by 255
// at gather time and converts sRGB -> linear under --color_space linear (nerf/provider.py:237,323-325; nerf/utils.py:640).  Here the bank is
// one packed RGBA8 word per pixel (R in the low byte; a 3-channel source stores alpha 255) and the decode is a gather from a [2,256] fp32
// table the host built with the reference's own torch expressions (row 0: R, G, B; row 1: alpha), so a decoded value has the bits of the
// torch statement by construction -- no device pow.  Ray arithmetic is batch_rays_kernel's (raymarching.hip), operand for operand; this
// file is compiled with -ffp-contract=off like the rest.
#include "n2m_common.hpp"

namespace {

__device__ __forceinline__ float4 decode_rgba8(uint32_t word, const float* __restrict__ lut) {
    return make_float4(lut[word & 255u], lut[(word >> 8) & 255u], lut[(word >> 16) & 255u], lut[256u + (word >> 24)]);
}

// The view a batch's uniform names: ONE expression for the batch kernels below and for batch_views_kernel, so that the view a ray read its
// pixel from and the view its appearance code is taken from cannot drift apart.
__device__ __forceinline__ uint32_t view_of_uniform(float u0, uint32_t V) { return min(V - 1u, (uint32_t)(u0 * (float)V)); }

// views_out[n] = the view ray n of the batch drawn from `u` reads (per-image appearance codes, --ind_dim; launched only then)
__global__ void __launch_bounds__(256) batch_views_kernel(const float* __restrict__ u /*[N,6]*/, uint32_t V, uint32_t N, int32_t* __restrict__ views_out) {
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n < N) views_out[n] = (int32_t)view_of_uniform(u[(size_t)n * 6], V);
}

// batch_rays_kernel with the ground truth read from the packed bank: one 4-byte load per ray instead of a 16-byte one
__global__ void __launch_bounds__(256)
batch_rays_u8_kernel(const float* __restrict__ poses /*[V,4,4]*/, const float* __restrict__ u /*[N,6]*/, uint32_t V, uint32_t N, uint32_t W,
                     uint32_t HW, float fx, float fy, float cx, float cy, const uint32_t* __restrict__ bank /*[V,HW]*/,
                     const float* __restrict__ lut /*[2,256]*/, const float* __restrict__ aabb, float min_near, float* __restrict__ rays_o,
                     float* __restrict__ rays_d, float* __restrict__ rgba, float* __restrict__ nears, float* __restrict__ fars,
                     float* __restrict__ noises, float* __restrict__ bg, int32_t* __restrict__ counter,
                     const float* __restrict__ cam_near_far /*[V,2] or NULL*/) {
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n == 0 && counter) counter[0] = 0;
    if (n >= N) return;
    const float* __restrict__ un = u + (size_t)n * 6;
    const uint32_t v = view_of_uniform(un[0], V), p = min(HW - 1u, (uint32_t)(un[1] * (float)HW));
    const float i = (float)(p % W) + 0.5f, j = (float)(p / W) + 0.5f;
    const float d0 = (i - cx) / fx, d1 = -(j - cy) / fy, d2 = -1.0f;
    const float* __restrict__ P = poses + (size_t)v * 16;
    float o[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d[k] = (d0 * P[4 * k] + d1 * P[4 * k + 1]) + d2 * P[4 * k + 2];
        o[k] = P[4 * k + 3];
        rays_d[(size_t)n * 3 + k] = d[k];
        rays_o[(size_t)n * 3 + k] = o[k];
    }
    *reinterpret_cast<float4*>(rgba + (size_t)n * 4) = decode_rgba8(bank[(size_t)v * HW + (size_t)p], lut);
    float tn, tf;
    n2m_near_far_of(o, d, aabb, min_near, tn, tf);
    if (cam_near_far) {
        tn = fmaxf(tn, cam_near_far[2 * v]);
        tf = fminf(tf, cam_near_far[2 * v + 1]);
    }
    nears[n] = tn; fars[n] = tf;
    noises[n] = un[2];
    if (bg) { bg[(size_t)n * 3] = un[3]; bg[(size_t)n * 3 + 1] = un[4]; bg[(size_t)n * 3 + 2] = un[5]; }
}

// batch_rays_u8_kernel for the keypoints of ONE view (sparse-depth supervision, nerf/colmap_provider.py:510-522): ray n goes through the
// centre of pixel coords[n] = (row, col) of that view instead of a pixel drawn from the uniforms; jitter and background still come from
// uniforms [K,6] (columns 2 and 3..5; columns 0, 1 are not read).  Also copies the keypoints' depth and weight into the batch.
__global__ void __launch_bounds__(256)
batch_rays_sparse_u8_kernel(const float* __restrict__ P /*[4,4] of the view*/, const float* __restrict__ u /*[K,6]*/, uint32_t K, uint32_t H,
                            uint32_t W, float fx, float fy, float cx, float cy, const uint32_t* __restrict__ bank /*[H W] of the view*/,
                            const float* __restrict__ lut /*[2,256]*/, const float* __restrict__ aabb, float min_near,
                            const int32_t* __restrict__ coords /*[K,2]*/, const float* __restrict__ kp_depth /*[K]*/,
                            const float* __restrict__ kp_weight /*[K]*/, float* __restrict__ rays_o, float* __restrict__ rays_d,
                            float* __restrict__ rgba, float* __restrict__ nears, float* __restrict__ fars, float* __restrict__ noises,
                            float* __restrict__ bg, float* __restrict__ gt_depth, float* __restrict__ depth_weight,
                            int32_t* __restrict__ counter, const float* __restrict__ near_far /*[2] of the view or NULL*/) {
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n == 0 && counter) counter[0] = 0;
    if (n >= K) return;
    const float* __restrict__ un = u + (size_t)n * 6;
    // (row, col) clamped to the image: the loader clips them already, the clamp keeps a hand-made table inside the bank
    const uint32_t row = (uint32_t)min(max(coords[(size_t)n * 2], 0), (int32_t)H - 1);
    const uint32_t col = (uint32_t)min(max(coords[(size_t)n * 2 + 1], 0), (int32_t)W - 1);
    const float i = (float)col + 0.5f, j = (float)row + 0.5f;
    const float d0 = (i - cx) / fx, d1 = -(j - cy) / fy, d2 = -1.0f;
    float o[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d[k] = (d0 * P[4 * k] + d1 * P[4 * k + 1]) + d2 * P[4 * k + 2];
        o[k] = P[4 * k + 3];
        rays_d[(size_t)n * 3 + k] = d[k];
        rays_o[(size_t)n * 3 + k] = o[k];
    }
    *reinterpret_cast<float4*>(rgba + (size_t)n * 4) = decode_rgba8(bank[(size_t)row * W + (size_t)col], lut);
    float tn, tf;
    n2m_near_far_of(o, d, aabb, min_near, tn, tf);
    if (near_far) {
        tn = fmaxf(tn, near_far[0]);
        tf = fminf(tf, near_far[1]);
    }
    nears[n] = tn; fars[n] = tf;
    noises[n] = un[2];
    if (bg) { bg[(size_t)n * 3] = un[3]; bg[(size_t)n * 3 + 1] = un[4]; bg[(size_t)n * 3 + 2] = un[5]; }
    gt_depth[n] = kp_depth[n];
    depth_weight[n] = kp_weight[n];
}

// batch_rays_u8_kernel + the dense-depth target of --enable_dense_depth (nerf/colmap_provider.py:552-553): gt_depth[n] is gathered from the
// fp32 depth bank [V,HW] at the index the colour word is read from.  Everything else is batch_rays_u8_kernel operand for operand.
__global__ void __launch_bounds__(256)
batch_rays_u8_depth_kernel(const float* __restrict__ poses /*[V,4,4]*/, const float* __restrict__ u /*[N,6]*/, uint32_t V, uint32_t N, uint32_t W,
                           uint32_t HW, float fx, float fy, float cx, float cy, const uint32_t* __restrict__ bank /*[V,HW]*/,
                           const float* __restrict__ depth_bank /*[V,HW]*/, const float* __restrict__ lut /*[2,256]*/,
                           const float* __restrict__ aabb, float min_near, float* __restrict__ rays_o, float* __restrict__ rays_d,
                           float* __restrict__ rgba, float* __restrict__ nears, float* __restrict__ fars, float* __restrict__ noises,
                           float* __restrict__ bg, float* __restrict__ gt_depth, int32_t* __restrict__ counter,
                           const float* __restrict__ cam_near_far /*[V,2] or NULL*/) {
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n == 0 && counter) counter[0] = 0;
    if (n >= N) return;
    const float* __restrict__ un = u + (size_t)n * 6;
    const uint32_t v = view_of_uniform(un[0], V), p = min(HW - 1u, (uint32_t)(un[1] * (float)HW));
    const float i = (float)(p % W) + 0.5f, j = (float)(p / W) + 0.5f;
    const float d0 = (i - cx) / fx, d1 = -(j - cy) / fy, d2 = -1.0f;
    const float* __restrict__ P = poses + (size_t)v * 16;
    float o[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d[k] = (d0 * P[4 * k] + d1 * P[4 * k + 1]) + d2 * P[4 * k + 2];
        o[k] = P[4 * k + 3];
        rays_d[(size_t)n * 3 + k] = d[k];
        rays_o[(size_t)n * 3 + k] = o[k];
    }
    const size_t at = (size_t)v * HW + (size_t)p;
    *reinterpret_cast<float4*>(rgba + (size_t)n * 4) = decode_rgba8(bank[at], lut);
    gt_depth[n] = depth_bank[at];
    float tn, tf;
    n2m_near_far_of(o, d, aabb, min_near, tn, tf);
    if (cam_near_far) {
        tn = fmaxf(tn, cam_near_far[2 * v]);
        tf = fminf(tf, cam_near_far[2 * v + 1]);
    }
    nears[n] = tn; fars[n] = tf;
    noises[n] = un[2];
    if (bg) { bg[(size_t)n * 3] = un[3]; bg[(size_t)n * 3 + 1] = un[4]; bg[(size_t)n * 3 + 2] = un[5]; }
}

// batch_rays_u8_kernel / batch_rays_u8_depth_kernel for a set with PER-VIEW intrinsics (nerf/colmap_provider.py:521,540, nerf/dtu_provider.py:265):
// ray n takes row v of intrinsics [V,4] = (fx, fy, cx, cy) -- one 16-byte load at the view index it already has; the table is V x 16 bytes
// and stays in cache.  depth_bank / gt_depth are both set or both NULL (the plain batch).  Everything else is batch_rays_u8_kernel operand
// for operand, so a table of equal rows gives its bits.
__global__ void __launch_bounds__(256)
batch_rays_u8_pv_kernel(const float* __restrict__ poses /*[V,4,4]*/, const float* __restrict__ u /*[N,6]*/, uint32_t V, uint32_t N, uint32_t W,
                        uint32_t HW, const float4* __restrict__ intrinsics /*[V] (fx, fy, cx, cy)*/, const uint32_t* __restrict__ bank /*[V,HW]*/,
                        const float* __restrict__ depth_bank /*[V,HW] or NULL*/, const float* __restrict__ lut /*[2,256]*/,
                        const float* __restrict__ aabb, float min_near, float* __restrict__ rays_o, float* __restrict__ rays_d,
                        float* __restrict__ rgba, float* __restrict__ nears, float* __restrict__ fars, float* __restrict__ noises,
                        float* __restrict__ bg, float* __restrict__ gt_depth /*[N] or NULL*/, int32_t* __restrict__ counter,
                        const float* __restrict__ cam_near_far /*[V,2] or NULL*/) {
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n == 0 && counter) counter[0] = 0;
    if (n >= N) return;
    const float* __restrict__ un = u + (size_t)n * 6;
    const uint32_t v = view_of_uniform(un[0], V), p = min(HW - 1u, (uint32_t)(un[1] * (float)HW));
    const float4 K = intrinsics[v];
    const float fx = K.x, fy = K.y, cx = K.z, cy = K.w;
    const float i = (float)(p % W) + 0.5f, j = (float)(p / W) + 0.5f;
    const float d0 = (i - cx) / fx, d1 = -(j - cy) / fy, d2 = -1.0f;
    const float* __restrict__ P = poses + (size_t)v * 16;
    float o[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d[k] = (d0 * P[4 * k] + d1 * P[4 * k + 1]) + d2 * P[4 * k + 2];
        o[k] = P[4 * k + 3];
        rays_d[(size_t)n * 3 + k] = d[k];
        rays_o[(size_t)n * 3 + k] = o[k];
    }
    const size_t at = (size_t)v * HW + (size_t)p;
    *reinterpret_cast<float4*>(rgba + (size_t)n * 4) = decode_rgba8(bank[at], lut);
    if (depth_bank) gt_depth[n] = depth_bank[at];
    float tn, tf;
    n2m_near_far_of(o, d, aabb, min_near, tn, tf);
    if (cam_near_far) {
        tn = fmaxf(tn, cam_near_far[2 * v]);
        tf = fminf(tf, cam_near_far[2 * v + 1]);
    }
    nears[n] = tn; fars[n] = tf;
    noises[n] = un[2];
    if (bg) { bg[(size_t)n * 3] = un[3]; bg[(size_t)n * 3 + 1] = un[4]; bg[(size_t)n * 3 + 2] = un[5]; }
}

// One view of the dense-depth bank (capture.dense_depth_fill): dst [H,W] = bilinear(src [h,w]) * scale + bias with cv2.INTER_LINEAR's
// geometry -- source coordinate (x + 0.5) * rx - 0.5 per axis (rx = w / W, ry = h / H as the host rounded them to fp32), the two taps of
// an axis clamped to the edge, fp32 weights, a + (b - a) * t per axis (columns first), so equal taps give their value exactly.  A thread
// per output pixel; the operand order is the torch statement's and the file is compiled without contraction: bit for bit.
__global__ void __launch_bounds__(256)
depth_bank_fill_kernel(const float* __restrict__ src /*[h,w]*/, uint32_t h, uint32_t w, uint32_t H, uint32_t W, float ry, float rx, float scale,
                       float bias, float* __restrict__ dst /*[H,W]*/) {
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= (size_t)H * W) return;
    const uint32_t y = (uint32_t)(n / W), x = (uint32_t)(n % W);
    const float sx = ((float)x + 0.5f) * rx - 0.5f, sy = ((float)y + 0.5f) * ry - 0.5f;
    const float fx0 = floorf(sx), fy0 = floorf(sy);
    const float tx = sx - fx0, ty = sy - fy0;
    const int32_t ix = (int32_t)fx0, iy = (int32_t)fy0;
    const size_t x0 = (size_t)min(max(ix, 0), (int32_t)w - 1), x1 = (size_t)min(max(ix + 1, 0), (int32_t)w - 1);
    const size_t y0 = (size_t)min(max(iy, 0), (int32_t)h - 1), y1 = (size_t)min(max(iy + 1, 0), (int32_t)h - 1);
    const float a = src[y0 * w + x0], b = src[y0 * w + x1], c = src[y1 * w + x0], e = src[y1 * w + x1];
    const float top = a + (b - a) * tx, bot = c + (e - c) * tx;
    dst[n] = (top + (bot - top) * ty) * scale + bias;
}

// One whole view at pixel stride s: output pixel (y, x) of the h x w grid is source pixel (y s, x s), its ray goes through that pixel's
// centre.  dirs (optional): safe_normalize(d) (nerf/utils.py) of every pixel repeated ssaa x ssaa times, i.e. the nearest upscale to
// [h ssaa, w ssaa] the stage-1 renderer shades with (nerf/renderer.py:821-828).
__global__ void __launch_bounds__(256)
capture_view_kernel(const float* __restrict__ pose /*[4,4]*/, uint32_t W, uint32_t h, uint32_t w, uint32_t s, float fx, float fy, float cx,
                    float cy, const uint32_t* __restrict__ bank /*[H W] of this view*/, const float* __restrict__ lut,
                    float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ rgba, float* __restrict__ dirs, uint32_t ssaa) {
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
    *reinterpret_cast<float4*>(rgba + (size_t)n * 4) = decode_rgba8(bank[(size_t)(y * s) * W + (size_t)(x * s)], lut);
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

// k x k integer box mean per channel, (sum + k k / 2) / (k k); rows and columns that do not fill a block are dropped.  grid.y = view.
__global__ void __launch_bounds__(256)
capture_box_downscale_kernel(const uint32_t* __restrict__ src /*[V,H,W]*/, uint32_t H, uint32_t W, uint32_t k, uint32_t h, uint32_t w,
                             uint32_t* __restrict__ dst /*[V,h,w]*/) {
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n >= h * w) return;
    const uint32_t y = n / w, x = n % w;
    const uint32_t* __restrict__ in = src + (size_t)blockIdx.y * H * W + (size_t)(y * k) * W + (size_t)(x * k);
    uint32_t sum[4] = {0u, 0u, 0u, 0u};
    for (uint32_t a = 0; a < k; ++a)
        for (uint32_t b = 0; b < k; ++b) {
            const uint32_t word = in[(size_t)a * W + b];
#pragma unroll
            for (int c = 0; c < 4; ++c) sum[c] += (word >> (8 * c)) & 255u;
        }
    const uint32_t kk = k * k, half = kk / 2;
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) out |= ((sum[c] + half) / kk) << (8 * c);
    dst[(size_t)blockIdx.y * h * w + n] = out;
}

}   // namespace

extern "C" int n2m_batch_rays_u8(const float* poses, const float* uniforms, uint32_t V, uint32_t N, uint32_t H, uint32_t W, float fx, float fy,
                                 float cx, float cy, const uint32_t* bank, const float* lut, const float* aabb, float min_near, float* rays_o,
                                 float* rays_d, float* rgba, float* nears, float* fars, float* noises, float* bg, int32_t* counter,
                                 const float* cam_near_far, void* stream) {
    N2M_NOTNULL(poses); N2M_NOTNULL(uniforms); N2M_NOTNULL(bank); N2M_NOTNULL(lut); N2M_NOTNULL(aabb); N2M_NOTNULL(rays_o); N2M_NOTNULL(rays_d);
    N2M_NOTNULL(rgba); N2M_NOTNULL(nears); N2M_NOTNULL(fars); N2M_NOTNULL(noises);
    N2M_REQUIRE(V >= 1 && H >= 1 && W >= 1 && (uint64_t)H * W < (1ull << 24), N2M_EINVAL,
                "batch_rays_u8: need V >= 1 and 1 <= H*W < 2^24 (pixel index from an fp32 uniform)");
    if (N == 0) return 0;
    batch_rays_u8_kernel<<<n2m_ceil_div(N, 256), 256, 0, (hipStream_t)stream>>>(poses, uniforms, V, N, W, H * W, fx, fy, cx, cy, bank, lut, aabb,
                                                                                min_near, rays_o, rays_d, rgba, nears, fars, noises, bg, counter,
                                                                                cam_near_far);
    N2M_CHECK_LAUNCH();
    return 0;
}

extern "C" int n2m_batch_rays_u8_depth(const float* poses, const float* uniforms, uint32_t V, uint32_t N, uint32_t H, uint32_t W, float fx, float fy,
                                       float cx, float cy, const uint32_t* bank, const float* depth_bank, const float* lut, const float* aabb,
                                       float min_near, float* rays_o, float* rays_d, float* rgba, float* nears, float* fars, float* noises, float* bg,
                                       float* gt_depth, int32_t* counter, const float* cam_near_far, void* stream) {
    N2M_NOTNULL(poses); N2M_NOTNULL(uniforms); N2M_NOTNULL(bank); N2M_NOTNULL(depth_bank); N2M_NOTNULL(lut); N2M_NOTNULL(aabb); N2M_NOTNULL(rays_o);
    N2M_NOTNULL(rays_d); N2M_NOTNULL(rgba); N2M_NOTNULL(nears); N2M_NOTNULL(fars); N2M_NOTNULL(noises); N2M_NOTNULL(gt_depth);
    N2M_REQUIRE(V >= 1 && H >= 1 && W >= 1 && (uint64_t)H * W < (1ull << 24), N2M_EINVAL,
                "batch_rays_u8_depth: need V >= 1 and 1 <= H*W < 2^24 (pixel index from an fp32 uniform)");
    if (N == 0) return 0;
    batch_rays_u8_depth_kernel<<<n2m_ceil_div(N, 256), 256, 0, (hipStream_t)stream>>>(poses, uniforms, V, N, W, H * W, fx, fy, cx, cy, bank, depth_bank,
                                                                                      lut, aabb, min_near, rays_o, rays_d, rgba, nears, fars, noises,
                                                                                      bg, gt_depth, counter, cam_near_far);
    N2M_CHECK_LAUNCH();
    return 0;
}

extern "C" int n2m_batch_rays_u8_pv(const float* poses, const float* uniforms, uint32_t V, uint32_t N, uint32_t H, uint32_t W, const float* intrinsics,
                                    const uint32_t* bank, const float* depth_bank, const float* lut, const float* aabb, float min_near,
                                    float* rays_o, float* rays_d, float* rgba, float* nears, float* fars, float* noises, float* bg, float* gt_depth,
                                    int32_t* counter, const float* cam_near_far, void* stream) {
    N2M_NOTNULL(poses); N2M_NOTNULL(uniforms); N2M_NOTNULL(intrinsics); N2M_NOTNULL(bank); N2M_NOTNULL(lut); N2M_NOTNULL(aabb); N2M_NOTNULL(rays_o);
    N2M_NOTNULL(rays_d); N2M_NOTNULL(rgba); N2M_NOTNULL(nears); N2M_NOTNULL(fars); N2M_NOTNULL(noises);
    N2M_REQUIRE((depth_bank == nullptr) == (gt_depth == nullptr), N2M_ENULL,
                "batch_rays_u8_pv: depth_bank and gt_depth are both set or both NULL, %s is NULL", depth_bank == nullptr ? "depth_bank" : "gt_depth");
    N2M_REQUIRE(V >= 1 && H >= 1 && W >= 1 && (uint64_t)H * W < (1ull << 24), N2M_EINVAL,
                "batch_rays_u8_pv: need V >= 1 and 1 <= H*W < 2^24 (pixel index from an fp32 uniform)");
    N2M_REQUIRE(((uintptr_t)intrinsics & 15u) == 0, N2M_EINVAL, "batch_rays_u8_pv: intrinsics [V,4] must be 16-byte aligned (one load per ray)");
    if (N == 0) return 0;
    batch_rays_u8_pv_kernel<<<n2m_ceil_div(N, 256), 256, 0, (hipStream_t)stream>>>(poses, uniforms, V, N, W, H * W,
                                                                                   reinterpret_cast<const float4*>(intrinsics), bank, depth_bank, lut,
                                                                                   aabb, min_near, rays_o, rays_d, rgba, nears, fars, noises, bg,
                                                                                   gt_depth, counter, cam_near_far);
    N2M_CHECK_LAUNCH();
    return 0;
}

extern "C" int n2m_batch_views(const float* uniforms, uint32_t V, uint32_t N, int32_t* views_out, void* stream) {
    N2M_NOTNULL(uniforms); N2M_NOTNULL(views_out);
    N2M_REQUIRE(V >= 1, N2M_EINVAL, "batch_views: need V >= 1");
    if (N == 0) return 0;
    batch_views_kernel<<<n2m_ceil_div(N, 256), 256, 0, (hipStream_t)stream>>>(uniforms, V, N, views_out);
    N2M_CHECK_LAUNCH();
    return 0;
}

extern "C" int n2m_depth_bank_fill(const float* src, uint32_t h, uint32_t w, uint32_t H, uint32_t W, float ry, float rx, float scale, float bias,
                                   float* dst, void* stream) {
    N2M_NOTNULL(src); N2M_NOTNULL(dst);
    N2M_REQUIRE(h >= 1 && w >= 1 && H >= 1 && W >= 1 && h < (1u << 24) && w < (1u << 24) && (uint64_t)H * W < (1ull << 32), N2M_EINVAL,
                "depth_bank_fill: need 1 <= h, w < 2^24 and 1 <= H*W < 2^32");
    depth_bank_fill_kernel<<<n2m_ceil_div((uint64_t)H * W, 256), 256, 0, (hipStream_t)stream>>>(src, h, w, H, W, ry, rx, scale, bias, dst);
    N2M_CHECK_LAUNCH();
    return 0;
}

// The keypoints [first, first + K) of the sparse-depth table belong to `view`; coords / kp_depth / kp_weight are the WHOLE table's arrays.
extern "C" int n2m_batch_rays_sparse_u8(const float* poses, const float* uniforms, uint32_t V, uint32_t view, uint32_t first, uint32_t K, uint32_t H,
                                        uint32_t W, float fx, float fy, float cx, float cy, const uint32_t* bank, const float* lut, const float* aabb,
                                        float min_near, const int32_t* coords, const float* kp_depth, const float* kp_weight, float* rays_o,
                                        float* rays_d, float* rgba, float* nears, float* fars, float* noises, float* bg, float* gt_depth,
                                        float* depth_weight, int32_t* counter, const float* cam_near_far, void* stream) {
    N2M_NOTNULL(poses); N2M_NOTNULL(uniforms); N2M_NOTNULL(bank); N2M_NOTNULL(lut); N2M_NOTNULL(aabb); N2M_NOTNULL(rays_o); N2M_NOTNULL(rays_d);
    N2M_NOTNULL(rgba); N2M_NOTNULL(nears); N2M_NOTNULL(fars); N2M_NOTNULL(noises); N2M_NOTNULL(coords); N2M_NOTNULL(kp_depth); N2M_NOTNULL(kp_weight);
    N2M_NOTNULL(gt_depth); N2M_NOTNULL(depth_weight);
    N2M_REQUIRE(view < V && H >= 1 && W >= 1 && (uint64_t)H * W < (1ull << 24) && (uint64_t)first + K < (1ull << 31), N2M_EINVAL,
                "batch_rays_sparse_u8: need view < V, 1 <= H*W < 2^24 and first + K < 2^31");
    if (K == 0) return 0;
    batch_rays_sparse_u8_kernel<<<n2m_ceil_div(K, 256), 256, 0, (hipStream_t)stream>>>(
        poses + (size_t)view * 16, uniforms, K, H, W, fx, fy, cx, cy, bank + (size_t)view * H * W, lut, aabb, min_near, coords + (size_t)first * 2,
        kp_depth + first, kp_weight + first, rays_o, rays_d, rgba, nears, fars, noises, bg, gt_depth, depth_weight, counter,
        cam_near_far ? cam_near_far + (size_t)view * 2 : nullptr);
    N2M_CHECK_LAUNCH();
    return 0;
}

extern "C" int n2m_capture_view(const float* poses, uint32_t V, uint32_t view, uint32_t H, uint32_t W, uint32_t stride, float fx, float fy, float cx,
                                float cy, const uint32_t* bank, const float* lut, float* rays_o, float* rays_d, float* rgba, float* dirs,
                                uint32_t ssaa, void* stream) {
    N2M_NOTNULL(poses); N2M_NOTNULL(bank); N2M_NOTNULL(lut); N2M_NOTNULL(rays_o); N2M_NOTNULL(rays_d); N2M_NOTNULL(rgba);
    N2M_REQUIRE(view < V && stride >= 1 && H >= 1 && W >= 1 && (uint64_t)H * W < (1ull << 24), N2M_EINVAL,
                "capture_view: need view < V, stride >= 1 and 1 <= H*W < 2^24");
    N2M_REQUIRE(dirs == nullptr || (ssaa >= 1 && ssaa <= 8), N2M_EINVAL, "capture_view: ssaa must be 1..8 when directions are asked for");
    const uint32_t h = H / stride, w = W / stride;
    if (h == 0 || w == 0) return 0;
    capture_view_kernel<<<n2m_ceil_div((uint64_t)h * w, 256), 256, 0, (hipStream_t)stream>>>(
        poses + (size_t)view * 16, W, h, w, stride, fx, fy, cx, cy, bank + (size_t)view * H * W, lut, rays_o, rays_d, rgba, dirs, ssaa);
    N2M_CHECK_LAUNCH();
    return 0;
}

extern "C" int n2m_capture_box_downscale(const uint32_t* src, uint32_t V, uint32_t H, uint32_t W, uint32_t k, uint32_t* dst, void* stream) {
    N2M_NOTNULL(src); N2M_NOTNULL(dst);
    N2M_REQUIRE(k >= 1 && k <= 64 && V <= 65535u && (uint64_t)H * W < (1ull << 32), N2M_EINVAL,
                "capture_box_downscale: need 1 <= k <= 64, V <= 65535 and H*W < 2^32");
    const uint32_t h = H / k, w = W / k;
    if (V == 0 || h == 0 || w == 0) return 0;
    capture_box_downscale_kernel<<<dim3(n2m_ceil_div((uint64_t)h * w, 256), V), 256, 0, (hipStream_t)stream>>>(src, H, W, k, h, w, dst);
    N2M_CHECK_LAUNCH();
    return 0;
}
