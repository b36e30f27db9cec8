// Camera-pose refinement for stage 0 (--optimize_poses; not a reference feature) -- n2m_pose_apply / n2m_pose_ray_grad / n2m_pose_view_grad
// of include/n2m_hip.h, DESIGN 4.31.
//
// A view's stored pose is camera-to-world [R0 | t0]; its correction delta = (omega, tau) gives [E(omega) R0 | t0 + tau] with
// E = exp([omega]x) = I + A [omega]x + B [omega]x^2,  A = sin th / th,  B = (1 - cos th) / th^2,  th = |omega|: a rotation about the camera
// centre in world axes, so a ray's origin o depends on tau alone and its direction is d = E R0 d_cam.  With the samples x_i = o + t_i d,
// g_i = dL/dx_i and h_i = dL/d(dirs_i):
//     g_o = sum_i g_i,   g_d = sum_i (t_i g_i + h_i),   dL/dtau = sum_rays g_o,   dL/domega = J_l(omega)^T sum_rays (d x g_d)
// J_l = I + B [omega]x + C [omega]x^2 the left Jacobian of SO(3), C = (th - sin th) / th^3  (E(omega + e) = exp([J_l e]x) E(omega) to first
// order, so d moves by (J_l e) x d).  t_i is the parameter the marcher formed x_i with: ts[i,0] - ts[i,1] (it writes t AFTER the step).
//
// The coefficients A, B, C are evaluated in double from the fp32 delta -- one thread per view, nothing to save -- and rounded once:
//   th <  kSeriesTheta: A = 1 - th^2/6 + th^4/120, B = 1/2 - th^2/24 + th^4/720, C = 1/6 - th^2/120 + th^4/5040
//   th >= kSeriesTheta: the closed forms
// At th = 1e-2 the series' first dropped terms are th^6/5040, th^6/20160 and th^6/60480 relative (< 2e-16), and the closed forms of B and C
// lose 2 / th^2 and 6 / th^2 ulps of double to cancellation (< 1.4e-11 relative): the two branches meet to 1e-11, five orders below an fp32
// ulp.  Any threshold between 1.2e-4 (the closed forms good to 2^-26) and 0.2 (the series good to 2^-26) would do.
//
// Mapping: n2m_pose_ray_grad is distortion.hip's -- one wave per ray, four waves per workgroup, a grid-stride loop over the rays, lanes
// stride the ray's samples (coalesced rows of grad_xyzs / grad_dirs / ts), six DPP wave sums.  n2m_pose_view_grad gives a wave to every
// view; its lanes stride ALL N rays and take the ones of that view (V x N int32 reads out of L2: 4096 rays x 200 views = 3 MB).  No LDS,
// no atomics; the order of every sum is fixed by (lane, index), so two runs give identical bits.  A permutation of the rays changes the
// order: the results then agree to rounding, not bitwise.
#include <algorithm>

#include "n2m_common.hpp"

namespace {

constexpr uint32_t kMaxBlocks = 2048;
constexpr double kSeriesTheta = N2M_POSE_SERIES_THETA;

struct PoseCoef { double A, B, C; };

__device__ __forceinline__ PoseCoef pose_coef(double wx, double wy, double wz) {
    const double t2 = wx * wx + wy * wy + wz * wz;
    PoseCoef c;
    if (t2 < kSeriesTheta * kSeriesTheta) {
        c.A = 1.0 - t2 / 6.0 + t2 * t2 / 120.0;
        c.B = 0.5 - t2 / 24.0 + t2 * t2 / 720.0;
        c.C = 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0;
    } else {
        const double th = sqrt(t2);
        c.A = sin(th) / th;
        c.B = (1.0 - cos(th)) / t2;
        c.C = (th - sin(th)) / (t2 * th);
    }
    return c;
}

// m = I + p [w]x + q [w]x^2, row-major
__device__ __forceinline__ void pose_matrix(double wx, double wy, double wz, double p, double q, double (&m)[9]) {
    const double xx = wx * wx, yy = wy * wy, zz = wz * wz, xy = wx * wy, xz = wx * wz, yz = wy * wz;
    m[0] = 1.0 - q * (yy + zz); m[1] = -p * wz + q * xy;    m[2] = p * wy + q * xz;
    m[3] = p * wz + q * xy;     m[4] = 1.0 - q * (xx + zz); m[5] = -p * wx + q * yz;
    m[6] = -p * wy + q * xz;    m[7] = p * wx + q * yz;     m[8] = 1.0 - q * (xx + yy);
}

__global__ void __launch_bounds__(256)
pose_apply_kernel(const float* __restrict__ poses0, const float* __restrict__ delta, uint32_t V, float* __restrict__ poses) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const float* p0 = poses0 + 16 * (size_t)v;
    const float* dl = delta + 6 * (size_t)v;
    float* p = poses + 16 * (size_t)v;
    const float wx = dl[0], wy = dl[1], wz = dl[2];
    float out[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) out[k] = p0[k];
    if (wx != 0.f || wy != 0.f || wz != 0.f) {              // omega == 0: R0 as it is
        const PoseCoef c = pose_coef(wx, wy, wz);
        double E[9];
        pose_matrix(wx, wy, wz, c.A, c.B, E);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                out[4 * r + k] = (float)(E[3 * r] * (double)p0[k] + E[3 * r + 1] * (double)p0[4 + k] + E[3 * r + 2] * (double)p0[8 + k]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
        if (dl[3 + r] != 0.f) out[4 * r + 3] = p0[4 * r + 3] + dl[3 + r];      // (t0 + 0 would turn a -0 into +0)
#pragma unroll
    for (int k = 0; k < 16; ++k) p[k] = out[k];
}

// Under opt.contract the marcher writes y = k(m) x for a world point x outside the unit box (m = max_a |x_a|, k = (2 - 1/m) / m, so
// max_a |y_a| = 2 - 1/m) and the field's gradient g arrives with respect to y.  The gradient with respect to x is
// J^T g = k g + e_a sign(x_a) k'(m) <x, g>,  k'(m) = -2/m^2 + 2/m^3,  a the axis of the maximum (the first one on a tie).
__device__ __forceinline__ void contract_vjp(float yx, float yy, float yz, float& gx, float& gy, float& gz) {
    const float ax = fabsf(yx), ay = fabsf(yy), az = fabsf(yz);
    const float mag = fmaxf(ax, fmaxf(ay, az));
    if (!(mag > 1.0f)) return;
    const float m = 1.0f / fmaxf(2.0f - mag, 1e-6f);
    const float k = (2.0f - 1.0f / m) / m;
    const float dk = -2.0f / (m * m) + 2.0f / (m * m * m);
    const float dot = (yx * gx + yy * gy + yz * gz) / k;          // <x, g>, x = y / k
    gx *= k; gy *= k; gz *= k;
    if (ax >= ay && ax >= az) gx += copysignf(1.0f, yx) * (dk * dot);
    else if (ay >= az) gy += copysignf(1.0f, yy) * (dk * dot);
    else gz += copysignf(1.0f, yz) * (dk * dot);
}

template <bool DIRS, bool CONTRACT>
__global__ void __launch_bounds__(256)
pose_ray_grad_kernel(const float* __restrict__ grad_xyzs, const float* __restrict__ grad_dirs, const float* __restrict__ xyzs,
                     const float* __restrict__ ts,
                     const int32_t* __restrict__ rays, const float* __restrict__ rays_d, uint32_t M, uint32_t N, float* __restrict__ ray6) {
    const int lane = threadIdx.x & 63;
    const uint32_t stride = gridDim.x * 4u;
    for (uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6); r < N; r += stride) {      // wave-uniform: every lane of a wave has one ray
        const int32_t off = rays[2 * r], cnt = rays[2 * r + 1];
        // a ray without samples, and a ray cut off by M (the rays the compositing kernels skip), gets six zeros
        const bool own = off >= 0 && cnt > 0 && (uint64_t)off + (uint64_t)cnt <= (uint64_t)M;
        const uint32_t n = own ? (uint32_t)cnt : 0u;
        float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
        for (uint32_t k = (uint32_t)lane; k < n; k += 64u) {
            const size_t i = (size_t)off + k;
            const float2 tt = *reinterpret_cast<const float2*>(ts + 2 * i);
            const float t = tt.x - tt.y;                                               // the t the marcher formed xyzs[i] with
            float gx = grad_xyzs[3 * i], gy = grad_xyzs[3 * i + 1], gz = grad_xyzs[3 * i + 2];
            if (CONTRACT) contract_vjp(xyzs[3 * i], xyzs[3 * i + 1], xyzs[3 * i + 2], gx, gy, gz);
            ox += gx; oy += gy; oz += gz;
            float hx = 0.f, hy = 0.f, hz = 0.f;
            if (DIRS) { hx = grad_dirs[3 * i]; hy = grad_dirs[3 * i + 1]; hz = grad_dirs[3 * i + 2]; }
            dx += t * gx + hx; dy += t * gy + hy; dz += t * gz + hz;
        }
        // (the loop above diverges in its last round; the sums below run with all 64 lanes again)
        ox = n2m_wave_sum(ox); oy = n2m_wave_sum(oy); oz = n2m_wave_sum(oz);
        dx = n2m_wave_sum(dx); dy = n2m_wave_sum(dy); dz = n2m_wave_sum(dz);
        if (lane == 0) {
            const float ax = rays_d[3 * (size_t)r], ay = rays_d[3 * (size_t)r + 1], az = rays_d[3 * (size_t)r + 2];
            float* o = ray6 + 6 * (size_t)r;
            o[0] = ox; o[1] = oy; o[2] = oz;
            // (n == 0: plain zeros, not the -0 a product with a negative direction component would leave)
            o[3] = n ? ay * dz - az * dy : 0.f; o[4] = n ? az * dx - ax * dz : 0.f; o[5] = n ? ax * dy - ay * dx : 0.f;
        }
    }
}

__global__ void __launch_bounds__(256)
pose_view_grad_kernel(const float* __restrict__ ray6, const int32_t* __restrict__ view, const float* __restrict__ delta, uint32_t N,
                      uint32_t V, float* __restrict__ grad_delta) {
    const int lane = threadIdx.x & 63;
    const uint32_t v = blockIdx.x * 4u + (threadIdx.x >> 6);                           // wave-uniform
    if (v >= V) return;
    float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // view[i] is compared, never used as an index: a value outside [0, V) matches no wave and its ray is skipped
    for (uint32_t i = (uint32_t)lane; i < N; i += 64u) {
        if ((uint32_t)view[i] != v) continue;
        const float* r = ray6 + 6 * (size_t)i;
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] += r[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = n2m_wave_sum(s[k]);
    if (lane == 0) {
        const float* dl = delta + 6 * (size_t)v;
        float* g = grad_delta + 6 * (size_t)v;
        const float wx = dl[0], wy = dl[1], wz = dl[2];
        const bool turned = wx != 0.f || wy != 0.f || wz != 0.f;
        if (turned && (s[3] != 0.f || s[4] != 0.f || s[5] != 0.f)) {       // (a view without a ray: plain zeros, not the -0 a product may leave)
            const PoseCoef c = pose_coef(wx, wy, wz);
            double J[9];
            pose_matrix(wx, wy, wz, c.B, c.C, J);
#pragma unroll
            for (int k = 0; k < 3; ++k) g[k] = (float)(J[k] * (double)s[3] + J[3 + k] * (double)s[4] + J[6 + k] * (double)s[5]);      // J_l^T
        } else {
            g[0] = s[3]; g[1] = s[4]; g[2] = s[5];
        }
        g[3] = s[0]; g[4] = s[1]; g[5] = s[2];
    }
}

}  // namespace

extern "C" int n2m_pose_apply(const float* poses0, const float* delta, uint32_t V, float* poses, void* stream) {
    N2M_REQUIRE(poses0 && delta && poses, N2M_EINVAL, "pose_apply: NULL tensor");
    N2M_REQUIRE(V > 0, N2M_EINVAL, "pose_apply: no views (V = 0)");
    pose_apply_kernel<<<n2m_ceil_div(V, 256), 256, 0, (hipStream_t)stream>>>(poses0, delta, V, poses);
    N2M_CHECK_LAUNCH();
    return 0;
}

extern "C" int n2m_pose_ray_grad(const float* grad_xyzs, const float* grad_dirs, const float* xyzs, const float* ts, const int32_t* rays,
                                 const float* rays_d, uint32_t M, uint32_t N, float* ray6, void* stream) {
    N2M_REQUIRE(grad_xyzs && ts && rays && rays_d && ray6, N2M_EINVAL, "pose_ray_grad: NULL tensor (only grad_dirs and xyzs may be NULL)");
    N2M_REQUIRE(M > 0 && N > 0, N2M_EINVAL, "pose_ray_grad: empty tensors (M = %u samples, N = %u rays; both must be > 0)", M, N);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t grid = std::min(n2m_ceil_div(N, 4), kMaxBlocks);
    if (grad_dirs && xyzs) pose_ray_grad_kernel<true, true><<<grid, 256, 0, s>>>(grad_xyzs, grad_dirs, xyzs, ts, rays, rays_d, M, N, ray6);
    else if (grad_dirs) pose_ray_grad_kernel<true, false><<<grid, 256, 0, s>>>(grad_xyzs, grad_dirs, xyzs, ts, rays, rays_d, M, N, ray6);
    else if (xyzs) pose_ray_grad_kernel<false, true><<<grid, 256, 0, s>>>(grad_xyzs, grad_dirs, xyzs, ts, rays, rays_d, M, N, ray6);
    else pose_ray_grad_kernel<false, false><<<grid, 256, 0, s>>>(grad_xyzs, grad_dirs, xyzs, ts, rays, rays_d, M, N, ray6);
    N2M_CHECK_LAUNCH();
    return 0;
}

extern "C" int n2m_pose_view_grad(const float* ray6, const int32_t* view, const float* delta, uint32_t N, uint32_t V, float* grad_delta,
                                  void* stream) {
    N2M_REQUIRE(ray6 && view && delta && grad_delta, N2M_EINVAL, "pose_view_grad: NULL tensor");
    N2M_REQUIRE(N > 0 && V > 0, N2M_EINVAL, "pose_view_grad: empty tensors (N = %u rays, V = %u views; both must be > 0)", N, V);
    pose_view_grad_kernel<<<n2m_ceil_div(V, 4), 256, 0, (hipStream_t)stream>>>(ray6, view, delta, N, V, grad_delta);
    N2M_CHECK_LAUNCH();
    return 0;
}
