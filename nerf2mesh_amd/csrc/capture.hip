// Captured image sets (nerf2mesh_amd/capture.py): the reference keeps its training images on the device as uint8 [N,H,W,3|4], divides by 255
// at gather time and converts sRGB -> linear under --color_space linear (nerf/provider.py:237,323-325; nerf/utils.py:640).  Here the bank is
// one packed RGBA8 word per pixel (R in the low byte; a 3-channel source stores alpha 255) and the decode is a gather from a [2,256] fp32
// table the host built with the reference's own torch expressions (row 0: R, G, B; row 1: alpha), so a decoded value has the bits of the
// torch statement by construction -- no device pow.  The batch kernel of the synthetic (fp32) bank lives here too; this file is compiled
// with -ffp-contract=off like the rest.
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

// A whole training batch in one launch: per ray the pixel choice, the ray (exactly as n2m_get_rays builds it, nerf/utils.py:242-290), the
// ground truth, near / far exactly as n2m_near_far_from_aabb + the per-view clamp of --enable_cam_near_far (nerf/renderer.py:689-691,
// colmap_provider.py:563-565: maximum / minimum), the march jitter u2 and the random background u3..u5 (nerf/utils.py:649-652); also clears
// the marcher's sample counter.  Seven small launches of the step's side stream are one (they ran 7-13 us EACH beside the optimizer update
// and delayed the march behind them).  The three things a batch can differ in:
//   the pixel         uniform mode: view = floor(u0 V), pixel = floor(u1 H W) (random_image_batch, nerf/provider.py:302-303);
//                     KP (sparse-depth supervision, nerf/colmap_provider.py:510-522): pixel coords[n] = (row, col) of the ONE view `view`,
//                     whose keypoint depth and weight are copied into the batch; columns 0, 1 of the uniforms are not read
//   the intrinsics    four scalars, or row v of a [V,4] table (per-view sets, colmap_provider.py:521,540, dtu_provider.py:265): one 16-byte
//                     load at the view index the ray already has; equal rows give the scalars' bits
//   the ground truth  U8: the packed bank through the LUT (one 4-byte load) + the optional depth gather of --enable_dense_depth
//                     (colmap_provider.py:552-553) at the same index; otherwise the fp32 images (one 16-byte load, nerf/provider.py:330)
// The struct carries no __restrict__, so every load of a ray is written in front of its first store.
struct BatchRaysK {
    const float* poses; const float* u; uint32_t V, N, H, W, HW; float fx, fy, cx, cy; const float4* intrinsics;
    const float* images; const uint32_t* bank; const float* lut; const float* depth_bank;
    const int32_t* coords; const float* kp_depth; const float* kp_weight; uint32_t view;
    const float* aabb; float min_near; const float* cam_near_far;
    float* rays_o; float* rays_d; float* rgba; float* nears; float* fars; float* noises; float* bg; float* gt_depth; float* depth_weight;
    int32_t* counter;
};

// ray n through the centre of pixel (row, col) of view v: everything the three modes share
template <bool U8>
__device__ __forceinline__ void batch_ray(const BatchRaysK& k, uint32_t n, uint32_t v, uint32_t col, uint32_t row, float fx, float fy, float cx,
                                          float cy) {
    const float* un = k.u + (size_t)n * 6;
    const float u2 = un[2], u3 = un[3], u4 = un[4], u5 = un[5];
    const float box[6] = {k.aabb[0], k.aabb[1], k.aabb[2], k.aabb[3], k.aabb[4], k.aabb[5]};
    const float i = (float)col + 0.5f, j = (float)row + 0.5f;
    const float d0 = (i - cx) / fx, d1 = -(j - cy) / fy, d2 = -1.0f;
    const float* P = k.poses + (size_t)v * 16;
    float o[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        d[c] = (d0 * P[4 * c] + d1 * P[4 * c + 1]) + d2 * P[4 * c + 2];
        o[c] = P[4 * c + 3];
    }
    const size_t at = (size_t)v * k.HW + ((size_t)row * k.W + col);
    float4 gt;
    float gtd = 0.0f;
    if constexpr (U8) {
        gt = decode_rgba8(k.bank[at], k.lut);
        if (k.depth_bank) gtd = k.depth_bank[at];
    } else {
        gt = *reinterpret_cast<const float4*>(k.images + at * 4);
    }
    float tn, tf;
    n2m_near_far_of(o, d, box, k.min_near, tn, tf);
    if (k.cam_near_far) {
        tn = fmaxf(tn, k.cam_near_far[2 * v]);
        tf = fminf(tf, k.cam_near_far[2 * v + 1]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        k.rays_d[(size_t)n * 3 + c] = d[c];
        k.rays_o[(size_t)n * 3 + c] = o[c];
    }
    *reinterpret_cast<float4*>(k.rgba + (size_t)n * 4) = gt;
    if constexpr (U8)
        if (k.depth_bank) k.gt_depth[n] = gtd;
    k.nears[n] = tn; k.fars[n] = tf;
    k.noises[n] = u2;
    if (k.bg) { k.bg[(size_t)n * 3] = u3; k.bg[(size_t)n * 3 + 1] = u4; k.bg[(size_t)n * 3 + 2] = u5; }
}

template <bool U8, bool KP>
__global__ void __launch_bounds__(256) batch_rays_kernel(const BatchRaysK k) {
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n >= k.N) return;
    if constexpr (KP) {
        const float depth = k.kp_depth[n], weight = k.kp_weight[n];
        // (row, col) clamped to the image: the loader clips them already, the clamp keeps a hand-made table inside the bank
        const uint32_t row = (uint32_t)min(max(k.coords[(size_t)n * 2], 0), (int32_t)k.H - 1);
        const uint32_t col = (uint32_t)min(max(k.coords[(size_t)n * 2 + 1], 0), (int32_t)k.W - 1);
        batch_ray<U8>(k, n, k.view, col, row, k.fx, k.fy, k.cx, k.cy);
        k.gt_depth[n] = depth;
        k.depth_weight[n] = weight;
    } else {
        const float* un = k.u + (size_t)n * 6;
        const uint32_t v = view_of_uniform(un[0], k.V), p = min(k.HW - 1u, (uint32_t)(un[1] * (float)k.HW));
        float fx = k.fx, fy = k.fy, cx = k.cx, cy = k.cy;
        if (k.intrinsics) {
            const float4 K = k.intrinsics[v];
            fx = K.x; fy = K.y; cx = K.z; cy = K.w;
        }
        batch_ray<U8>(k, n, v, p % k.W, p / k.W, fx, fy, cx, cy);
    }
    if (n == 0 && k.counter) k.counter[0] = 0;
}

// Patch mode (--patch_size P, nerf/utils.py:253-267): the batch is B = N / P^2 random P x P patches, ray n the pixel (k / P, k % P) of
// patch p = n / P^2, k = n % P^2 (meshgrid 'ij' order: rgba [N,4] viewed as [B,P,P,4] is the patches, row-major).  The three draws of a
// patch come from the uniforms of its first two rays, f = p P^2: the view from u[f,0] through view_of_uniform, the top row from u[f,1] over
// H - P start rows and the left column from u[f+1,1] over W - P start columns (randint(0, H - P), upper end excluded: the last start row and
// column are never drawn, as in the reference).  Columns 2..5 stay per ray.  Everything after the pixel choice is batch_ray.
template <bool U8>
__global__ void __launch_bounds__(256) batch_rays_patch_kernel(const BatchRaysK k, uint32_t P, uint32_t PP) {
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n >= k.N) return;
    const uint32_t p = n / PP, q = n - p * PP;
    const float* uf = k.u + (size_t)p * PP * 6;
    const uint32_t v = view_of_uniform(uf[0], k.V);
    const uint32_t i0 = min(k.H - P - 1u, (uint32_t)(uf[1] * (float)(k.H - P)));
    const uint32_t j0 = min(k.W - P - 1u, (uint32_t)(uf[7] * (float)(k.W - P)));
    float fx = k.fx, fy = k.fy, cx = k.cx, cy = k.cy;
    if (k.intrinsics) {
        const float4 K = k.intrinsics[v];
        fx = K.x; fy = K.y; cx = K.z; cy = K.w;
    }
    batch_ray<U8>(k, n, v, j0 + q % P, i0 + q / P, fx, fy, cx, cy);
    if (n == 0 && k.counter) k.counter[0] = 0;
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

// ---------------------------------------------------------------------------------------------- lens undistortion (capture.undistort_bank)
// The forward lens model of COLMAP's camera models (https://colmap.github.io/cameras.html): ideal normalised (x, y), y down, -> distorted
// normalised (xd, yd).  Mirror of capture.lens_distort_f32, operation for operation: fp32, no contraction, the order below.
//   N2M_LENS_BROWN (row = k1, k2, p1, p2, 0...: SIMPLE_RADIAL, RADIAL, OPENCV and, all zero, the pinhole models)
//     xx = x x, yy = y y, r2 = xx + yy, r4 = r2 r2, xy = x y, radial = k1 r2 + k2 r4
//     xd = x + ((x radial + (p1 xy + p1 xy)) + p2 (r2 + (xx + xx)))
//     yd = y + ((y radial + (p2 xy + p2 xy)) + p1 (r2 + (yy + yy)))
//   N2M_LENS_FISHEYE (row = k1, k2, k3, k4, 0...: OPENCV_FISHEYE)
//     r = sqrt(r2) (correctly rounded), theta = atan(r) by lens_atan below, t2 = theta theta, t4 = t2 t2, t6 = t4 t2, t8 = t4 t4
//     thetad = theta (1 + (((k1 t2 + k2 t4) + k3 t6) + k4 t8)), scale = thetad / r (1 where r < 1e-8), xd = x scale, yd = y scale
// lens_atan, r >= 0: a library atanf has no stated rounding, so the arc tangent is spelled out in +, -, *, / (each correctly rounded on
// both sides): t = 1 / r where r > 1; z = (t - 1) / (t + 1) where t > tan(pi / 8); the Taylor series of atan to z^17 by Horner in z^2
// (|z| <= tan(pi / 8): the first dropped term is below 3e-9); + pi / 4 where reduced; pi / 2 - (that) where inverted.
constexpr float LENS_TAN_PI_8 = 0.41421356237309503f, LENS_PI_4 = 0.78539816339744831f, LENS_PI_2 = 1.5707963267948966f;

__device__ __forceinline__ float lens_atan(float r) {
    const bool inv = r > 1.0f;
    const float t = inv ? 1.0f / r : r;
    const bool red = t > LENS_TAN_PI_8;
    const float z = red ? (t - 1.0f) / (t + 1.0f) : t;
    const float z2 = z * z;
    float p = (float)(1.0 / 17.0);
    p = p * z2 - (float)(1.0 / 15.0);
    p = p * z2 + (float)(1.0 / 13.0);
    p = p * z2 - (float)(1.0 / 11.0);
    p = p * z2 + (float)(1.0 / 9.0);
    p = p * z2 - (float)(1.0 / 7.0);
    p = p * z2 + (float)(1.0 / 5.0);
    p = p * z2 - (float)(1.0 / 3.0);
    p = p * z2 + 1.0f;
    float a = p * z;
    if (red) a = a + LENS_PI_4;
    return inv ? LENS_PI_2 - a : a;
}

__device__ __forceinline__ void lens_distort(uint32_t model, const float4 ka, float x, float y, float& xd, float& yd) {
    const float xx = x * x, yy = y * y, r2 = xx + yy;
    if (model == N2M_LENS_FISHEYE) {
        const float r = sqrtf(r2);
        const float th = lens_atan(r);
        const float t2 = th * th, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
        const float thd = th * (1.0f + (((ka.x * t2 + ka.y * t4) + ka.z * t6) + ka.w * t8));
        const float scale = r < 1e-8f ? 1.0f : thd / r;
        xd = x * scale; yd = y * scale;
        return;
    }
    const float r4 = r2 * r2, xy = x * y;
    const float radial = ka.x * r2 + ka.y * r4;
    const float a = ka.z * xy, b = ka.w * xy;
    xd = x + ((x * radial + (a + a)) + ka.w * (r2 + (xx + xx)));
    yd = y + ((y * radial + (b + b)) + ka.z * (r2 + (yy + yy)));
}

// One output pixel of every view: normalised coordinates from the OUTPUT camera (pixel centre (col + 0.5, row + 0.5), the convention of
// capture.rays_from_pixels), the lens model, the SOURCE camera: u = fx xd + cx, v = fy yd + cy (continuous, pixel c covers [c, c + 1)).
//   colour (DEPTH = false): sx = u - 0.5, sy = v - 0.5, taps floor and floor + 1 clamped to the image, weights tx = sx - floor(sx), ty likewise; per
//     8-bit channel top = a + (b - a) tx, bot = c + (e - c) tx, val = top + (bot - top) ty, byte = clamp(floor(val + 0.5), 0, 255).  One word load per tap.
//   depth (DEPTH = true): the texel that contains (u, v): (floor(v), floor(u)) clamped -- never a mix of two depths.
// A thread per output pixel, consecutive lanes on consecutive columns (the taps of a wave fall in a few lines); grid.y = view.  The
// per-view rows are wave-uniform: three 16-byte loads (the second half of a lens row is reserved, no model here reads it).
struct UndistortK {
    const void* src; void* dst; uint32_t H, W, model; uint32_t stride;      // stride: 1 = tables of V rows, 0 = one row for every view
    const float4* src_k; const float4* out_k; const float4* lens;           // [V or 1] x (1, 1, 2) float4
};

template <bool DEPTH>
__global__ void __launch_bounds__(256) capture_undistort_kernel(const UndistortK k) {
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    const uint32_t HW = k.H * k.W;
    if (n >= HW) return;
    const uint32_t v = blockIdx.y, t = v * k.stride;
    const float4 S = k.src_k[t], O = k.out_k[t], ka = k.lens[2 * t];
    const uint32_t row = n / k.W, col = n % k.W;
    const float i = (float)col + 0.5f, j = (float)row + 0.5f;
    const float x = (i - O.z) / O.x, y = (j - O.w) / O.y;
    float xd, yd;
    lens_distort(k.model, ka, x, y, xd, yd);
    const float u = S.x * xd + S.z, w = S.y * yd + S.w;
    const int32_t Wm = (int32_t)k.W - 1, Hm = (int32_t)k.H - 1;
    const size_t base = (size_t)v * HW;
    if constexpr (DEPTH) {
        // clamped as floats (fmaxf drops a NaN), then converted: every index is inside the plane whatever the rows hold
        const size_t ix = (size_t)fminf(fmaxf(floorf(u), 0.0f), (float)Wm), iy = (size_t)fminf(fmaxf(floorf(w), 0.0f), (float)Hm);
        const float* __restrict__ in = reinterpret_cast<const float*>(k.src) + base;
        reinterpret_cast<float*>(k.dst)[base + n] = in[iy * k.W + ix];
    } else {
        const float sx = u - 0.5f, sy = w - 0.5f;
        const float fx0 = floorf(sx), fy0 = floorf(sy);
        const float tx = sx - fx0, ty = sy - fy0;
        // clamped to [-1, size] as floats (fmaxf drops a NaN), then converted: the four taps are inside the image whatever the rows hold
        const int32_t ix = (int32_t)fminf(fmaxf(fx0, -1.0f), (float)k.W), iy = (int32_t)fminf(fmaxf(fy0, -1.0f), (float)k.H);
        const size_t x0 = (size_t)min(max(ix, 0), Wm), x1 = (size_t)min(ix + 1, Wm);
        const size_t y0 = (size_t)min(max(iy, 0), Hm), y1 = (size_t)min(iy + 1, Hm);
        const uint32_t* __restrict__ in = reinterpret_cast<const uint32_t*>(k.src) + base;
        const uint32_t wa = in[y0 * k.W + x0], wb = in[y0 * k.W + x1], wc = in[y1 * k.W + x0], we = in[y1 * k.W + x1];
        uint32_t out = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float a = (float)((wa >> (8 * c)) & 255u), b = (float)((wb >> (8 * c)) & 255u);
            const float cc = (float)((wc >> (8 * c)) & 255u), e = (float)((we >> (8 * c)) & 255u);
            const float top = a + (b - a) * tx, bot = cc + (e - cc) * tx;
            const float val = floorf((top + (bot - top) * ty) + 0.5f);
            out |= (uint32_t)fminf(fmaxf(val, 0.0f), 255.0f) << (8 * c);
        }
        reinterpret_cast<uint32_t*>(k.dst)[base + n] = out;
    }
}

}   // namespace

extern "C" int n2m_capture_undistort(const N2mUndistort* d, void* stream) {
    N2M_NOTNULL(d);
    N2M_NOTNULL(d->src); N2M_NOTNULL(d->dst); N2M_NOTNULL(d->src_intrinsics); N2M_NOTNULL(d->out_intrinsics); N2M_NOTNULL(d->lens);
    N2M_REQUIRE(d->src != d->dst, N2M_EINVAL, "capture_undistort: out of place only, src and dst are the same buffer");
    N2M_REQUIRE(d->model == N2M_LENS_BROWN || d->model == N2M_LENS_FISHEYE, N2M_EINVAL, "capture_undistort: model must be N2M_LENS_BROWN or N2M_LENS_FISHEYE");
    N2M_REQUIRE(d->V <= 65535u && d->H >= 1 && d->W >= 1 && d->H < (1u << 24) && d->W < (1u << 24) && (uint64_t)d->H * d->W < (1ull << 31), N2M_EINVAL,
                "capture_undistort: need V <= 65535, 1 <= H, W < 2^24 and H*W < 2^31");
    N2M_REQUIRE((((uintptr_t)d->src_intrinsics | (uintptr_t)d->out_intrinsics | (uintptr_t)d->lens) & 15u) == 0, N2M_EINVAL,
                "capture_undistort: the intrinsics and lens rows must be 16-byte aligned");
    if (d->V == 0) return 0;
    const UndistortK k{d->src, d->dst, d->H, d->W, d->model, d->per_view ? 1u : 0u, reinterpret_cast<const float4*>(d->src_intrinsics),
                       reinterpret_cast<const float4*>(d->out_intrinsics), reinterpret_cast<const float4*>(d->lens)};
    const dim3 grid(n2m_ceil_div((uint64_t)d->H * d->W, 256), d->V);
    if (d->depth) capture_undistort_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(k);
    else capture_undistort_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(k);
    N2M_CHECK_LAUNCH();
    return 0;
}

// P == 0: the pixel / keypoint batch of n2m_batch_rays; P >= 2: the patch batch of n2m_batch_rays_patch.  One set of checks for both.
static int batch_rays(const N2mBatchRays* d, uint32_t P, bool patch, void* stream) {
    N2M_NOTNULL(d);
    N2M_NOTNULL(d->poses); N2M_NOTNULL(d->uniforms); N2M_NOTNULL(d->aabb); N2M_NOTNULL(d->rays_o); N2M_NOTNULL(d->rays_d); N2M_NOTNULL(d->rgba);
    N2M_NOTNULL(d->nears); N2M_NOTNULL(d->fars); N2M_NOTNULL(d->noises);
    const bool u8 = d->bank != nullptr, kp = d->coords != nullptr;
    N2M_REQUIRE(u8 || d->images != nullptr, N2M_ENULL, "batch_rays: no ground truth, images (fp32) and bank (RGBA8 words) are both NULL");
    N2M_REQUIRE(!u8 || d->images == nullptr, N2M_EINVAL, "batch_rays: images (fp32) and bank (RGBA8 words) are mutually exclusive");
    N2M_REQUIRE(d->intrinsics != nullptr || (d->fx != 0.f && d->fy != 0.f), N2M_EINVAL, "batch_rays: intrinsics is NULL and the scalar fx / fy are zero");
    if (u8) N2M_NOTNULL(d->lut);
    N2M_REQUIRE(d->V >= 1 && d->H >= 1 && d->W >= 1 && (uint64_t)d->H * d->W < (1ull << 24), N2M_EINVAL,
                "batch_rays: need V >= 1 and 1 <= H*W < 2^24 (pixel index from an fp32 uniform)");
    if (kp) {       // the keypoints [first, first + N) of the sparse-depth table belong to `view`; coords / kp_depth / kp_weight are the WHOLE table's arrays
        N2M_NOTNULL(d->bank); N2M_NOTNULL(d->kp_depth); N2M_NOTNULL(d->kp_weight); N2M_NOTNULL(d->gt_depth); N2M_NOTNULL(d->depth_weight);
        N2M_REQUIRE(d->intrinsics == nullptr && d->depth_bank == nullptr, N2M_EINVAL,
                    "batch_rays: a keypoint batch takes its view's four scalar intrinsics and its depth from the keypoints");
        N2M_REQUIRE(d->view < d->V && (uint64_t)d->first + d->N < (1ull << 31), N2M_EINVAL, "batch_rays: need view < V and first + K < 2^31");
    } else {
        N2M_REQUIRE((d->depth_bank == nullptr) == (d->gt_depth == nullptr), N2M_ENULL,
                    "batch_rays: depth_bank and gt_depth are both set or both NULL, %s is NULL", d->depth_bank == nullptr ? "depth_bank" : "gt_depth");
        N2M_REQUIRE(d->depth_bank == nullptr || u8, N2M_EUNSUPPORTED, "batch_rays: the depth gather is built beside the RGBA8 bank only");
        N2M_REQUIRE(((uintptr_t)d->intrinsics & 15u) == 0, N2M_EINVAL, "batch_rays: intrinsics [V,4] must be 16-byte aligned (one load per ray)");
    }
    if (patch) {
        N2M_REQUIRE(!kp, N2M_EUNSUPPORTED, "batch_rays_patch: keypoint batches (coords != NULL) have no patch mode");
        N2M_REQUIRE(P >= 2 && P < d->H && P < d->W, N2M_EINVAL, "batch_rays_patch: need 2 <= P < H and P < W, got P = %u on %u x %u", P, d->H, d->W);
        N2M_REQUIRE(d->N % (P * P) == 0, N2M_EINVAL, "batch_rays_patch: N = %u is not a multiple of P^2 = %u", d->N, P * P);
    }
    if (d->N == 0) return 0;
    const BatchRaysK k{d->poses, d->uniforms, d->V, d->N, d->H, d->W, d->H * d->W, d->fx, d->fy, d->cx, d->cy,
                       reinterpret_cast<const float4*>(d->intrinsics), d->images, d->bank, d->lut, d->depth_bank,
                       kp ? d->coords + (size_t)d->first * 2 : nullptr, kp ? d->kp_depth + d->first : nullptr, kp ? d->kp_weight + d->first : nullptr,
                       d->view, d->aabb, d->min_near, d->cam_near_far, d->rays_o, d->rays_d, d->rgba, d->nears, d->fars, d->noises, d->bg,
                       d->gt_depth, d->depth_weight, d->counter};
    const dim3 grid(n2m_ceil_div(d->N, 256));
    if (patch) {
        if (u8) batch_rays_patch_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(k, P, P * P);
        else batch_rays_patch_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(k, P, P * P);
    } else if (kp) batch_rays_kernel<true, true><<<grid, 256, 0, (hipStream_t)stream>>>(k);
    else if (u8) batch_rays_kernel<true, false><<<grid, 256, 0, (hipStream_t)stream>>>(k);
    else batch_rays_kernel<false, false><<<grid, 256, 0, (hipStream_t)stream>>>(k);
    N2M_CHECK_LAUNCH();
    return 0;
}

extern "C" int n2m_batch_rays(const N2mBatchRays* d, void* stream) { return batch_rays(d, 0, false, stream); }

extern "C" int n2m_batch_rays_patch(const N2mBatchRays* d, uint32_t P, void* stream) { return batch_rays(d, P, true, stream); }

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
