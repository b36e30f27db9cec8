// Distortion loss on the ray weights (mip-NeRF 360, eq. 15) over packed, variable-length rays -- n2m_distortion_forward / _backward of
// include/n2m_hip.h, DESIGN 4.30.  Not a reference operator: nerf2mesh dropped the term its ancestor carried.
//
// Per ray, samples i = 0 .. n-1 in marching order, weight w_i, interval [t_i - dt_i, t_i] (the marcher writes t AFTER the step) mapped to
// s(t) = (g(t) - g(near)) / (g(far) - g(near)), g(t) = t (space 0) or 1 / t (space 1); m_i the interval's midpoint in s, d_i its length:
//     L_ray       = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i
//                 = 2 sum_i w_i (m_i W_<i - S_<i) + (1/3) sum_i w_i^2 d_i            (m is non-decreasing along a ray in both spaces)
//     dL_ray/dw_i = 2 [m_i (W_<i - W_>i) - S_<i + S_>i] + (2/3) w_i d_i
// with the exclusive prefix sums W_<i = sum_{j<i} w_j, S_<i = sum_{j<i} w_j m_j and W_>i = W - W_<i - w_i, S_>i = S - S_<i - w_i m_i.
// Only differences of midpoints enter, so the kernels measure m from the start of the ray's first interval (dist_interval below).
//
// Mapping: composite_train_fwd_kernel's -- one wave per ray, four waves per workgroup -- with a grid-stride loop over the rays.  A ray is
// taken in chunks of 64 consecutive samples (coalesced loads of weights and ts), (w, w m) go through one wave scan each and a two-float
// carry crosses the chunks in registers.  No LDS, no atomics; the order of every sum is fixed by the sample index alone, so two runs give
// identical bits.
#include <algorithm>

#include "n2m_common.hpp"

namespace {

constexpr uint32_t kMaxBlocks = 2048;          // 8 workgroups of 4 waves per CU; beyond that the grid-stride loop takes over

struct DistRay {
    uint32_t off, cnt;      // the samples the term is formed over (cnt == 0: none)
    uint32_t zero_end;      // backward: rows [off, zero_end) are owned by the ray but carry no term and get an exact zero (0: none)
    float t_ref, den, c;    // the lower end of the ray's first interval; far - near; disparity: far * near / t_ref
};

// A ray without samples owns nothing.  A ray cut off by M (off + cnt > M, skipped by the compositing kernels as well) and a degenerate ray
// (not far > near: the normalised coordinate does not exist) contribute 0 loss and 0 gradient; what they own inside [0, M) is zeroed.
__device__ __forceinline__ DistRay dist_ray(const float* __restrict__ ts, const int32_t* __restrict__ rays, const float* __restrict__ nears,
                                            const float* __restrict__ fars, uint32_t r, uint32_t M) {
    DistRay d = {0u, 0u, 0u, 1.f, 1.f, 1.f};
    const int32_t off = rays[2 * r], cnt = rays[2 * r + 1];
    if (off < 0 || cnt <= 0 || (uint32_t)off >= M) return d;
    d.off = (uint32_t)off;
    const uint64_t end = (uint64_t)off + (uint64_t)cnt;
    const float near = nears[r], far = fars[r];
    if (end > (uint64_t)M || !(far > near)) {
        d.zero_end = end > (uint64_t)M ? M : (uint32_t)end;
        return d;
    }
    d.cnt = (uint32_t)cnt;
    const float2 first = *reinterpret_cast<const float2*>(ts + 2 * (size_t)off);
    d.t_ref = first.x - first.y;
    d.den = far - near;
    d.c = far * near / d.t_ref;
    return d;
}

// Midpoint and length of the interval [t - dt, t] in the coordinate u(t) = s(t) - s(t_ref), t_ref the lower end of the ray's first
// interval.  The term and its gradient only hold differences of midpoints, so the shift changes neither; it is there for the arithmetic:
//   * m_i (W_<i - W_>i) - S_<i + S_>i cancels down from |m| W to (spread of the ray's samples) W.  Samples that sit together far from
//     the ray's near end -- a ray that crosses empty space first, the usual case on a trained scene -- lose spread / |m| of the fp32
//     digits with s itself (2e-4 of the gradient on real batches) and none with u, which starts at 0 where the samples start;
//   * u comes from t - t_ref, never from a difference of two values of g: linear u = (t - t_ref) / (far - near); disparity
//     (1/t - 1/t_ref) / (1/far - 1/near) = (t - t_ref) / (far - near) * far near / (t t_ref).
template <int SPACE>
__device__ __forceinline__ void dist_interval(float t, float dt, const DistRay& ray, float& m, float& d) {
    const float b = t - ray.t_ref;
    float lo = (b - dt) / ray.den, hi = b / ray.den;
    if (SPACE) {
        lo *= ray.c / (t - dt);
        hi *= ray.c / t;
    }
    m = (lo + hi) * 0.5f;
    d = fabsf(hi - lo);
}

template <int SPACE>
__global__ void __launch_bounds__(256)
distortion_fwd_kernel(const float* __restrict__ weights, const float* __restrict__ ts, const int32_t* __restrict__ rays,
                      const float* __restrict__ nears, const float* __restrict__ fars, uint32_t M, uint32_t N,
                      float* __restrict__ loss_ray, float* __restrict__ totals) {
    const int lane = threadIdx.x & 63;
    const uint32_t stride = gridDim.x * 4u;
    for (uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6); r < N; r += stride) {      // wave-uniform: every lane of a wave has one ray
        const DistRay ray = dist_ray(ts, rays, nears, fars, r, M);
        float acc = 0.f, carry_W = 0.f, carry_S = 0.f;
        for (uint32_t base = 0; base < ray.cnt; base += 64u) {
            const uint32_t k = base + (uint32_t)lane;
            float w = 0.f, m = 0.f, d = 0.f;
            if (k < ray.cnt) {
                const size_t i = (size_t)ray.off + k;
                const float2 tt = *reinterpret_cast<const float2*>(ts + 2 * i);
                w = weights[i];
                dist_interval<SPACE>(tt.x, tt.y, ray, m, d);
            }
            const float incl_W = n2m_wave_scan_add(w, lane), incl_S = n2m_wave_scan_add(w * m, lane);
            const float W_lt = carry_W + n2m_lane_below(incl_W, 0.f), S_lt = carry_S + n2m_lane_below(incl_S, 0.f);
            acc += 2.0f * w * (m * W_lt - S_lt) + (w * w * d) / 3.0f;
            carry_W += n2m_lane63(incl_W);
            carry_S += n2m_lane63(incl_S);
        }
        acc = n2m_wave_sum(acc);
        if (lane == 0) {
            loss_ray[r] = acc;
            totals[2 * r] = carry_W;
            totals[2 * r + 1] = carry_S;
        }
    }
}

template <int SPACE>
__global__ void __launch_bounds__(256)
distortion_bwd_kernel(const float* __restrict__ weights, const float* __restrict__ ts, const int32_t* __restrict__ rays,
                      const float* __restrict__ nears, const float* __restrict__ fars, const float* __restrict__ totals,
                      const float* __restrict__ grad_ray, uint32_t M, uint32_t N, float* __restrict__ grad_weights) {
    const int lane = threadIdx.x & 63;
    const uint32_t stride = gridDim.x * 4u;
    for (uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6); r < N; r += stride) {
        const DistRay ray = dist_ray(ts, rays, nears, fars, r, M);
        for (size_t i = (size_t)ray.off + (size_t)lane; i < (size_t)ray.zero_end; i += 64u) grad_weights[i] = 0.f;
        if (ray.cnt == 0u) continue;
        const float W = totals[2 * r], S = totals[2 * r + 1], g = grad_ray[r];
        float carry_W = 0.f, carry_S = 0.f;
        for (uint32_t base = 0; base < ray.cnt; base += 64u) {
            const uint32_t k = base + (uint32_t)lane;
            const bool valid = k < ray.cnt;
            const size_t i = (size_t)ray.off + k;
            float w = 0.f, m = 0.f, d = 0.f;
            if (valid) {
                const float2 tt = *reinterpret_cast<const float2*>(ts + 2 * i);
                w = weights[i];
                dist_interval<SPACE>(tt.x, tt.y, ray, m, d);
            }
            const float wm = w * m;
            const float incl_W = n2m_wave_scan_add(w, lane), incl_S = n2m_wave_scan_add(wm, lane);
            const float W_lt = carry_W + n2m_lane_below(incl_W, 0.f), S_lt = carry_S + n2m_lane_below(incl_S, 0.f);
            const float W_gt = W - W_lt - w, S_gt = S - S_lt - wm;
            if (valid) grad_weights[i] = g * (2.0f * (m * (W_lt - W_gt) - S_lt + S_gt) + (2.0f * w * d) / 3.0f);
            carry_W += n2m_lane63(incl_W);
            carry_S += n2m_lane63(incl_S);
        }
    }
}

int check_distortion(const char* who, uint32_t M, uint32_t N, int space) {
    N2M_REQUIRE(M > 0 && N > 0, N2M_EINVAL, "%s: empty tensors (M = %u samples, N = %u rays; both must be > 0)", who, M, N);
    N2M_REQUIRE(space == N2M_DISTORT_LINEAR || space == N2M_DISTORT_DISPARITY, N2M_EINVAL, "%s: space must be 0 (linear) or 1 (disparity), got %d",
                who, space);
    return 0;
}

}  // namespace

extern "C" int n2m_distortion_forward(const float* weights, const float* ts, const int32_t* rays, const float* nears, const float* fars,
                                      uint32_t M, uint32_t N, int space, float* loss_ray, float* totals, void* stream) {
    N2M_REQUIRE(weights && ts && rays && nears && fars && loss_ray && totals, N2M_ENULL, "distortion_forward: NULL tensor");
    if (int rc = check_distortion("distortion_forward", M, N, space)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t grid = std::min(n2m_ceil_div(N, 4), kMaxBlocks);
    if (space == N2M_DISTORT_LINEAR) distortion_fwd_kernel<0><<<grid, 256, 0, s>>>(weights, ts, rays, nears, fars, M, N, loss_ray, totals);
    else distortion_fwd_kernel<1><<<grid, 256, 0, s>>>(weights, ts, rays, nears, fars, M, N, loss_ray, totals);
    N2M_CHECK_LAUNCH();
    return 0;
}

extern "C" int n2m_distortion_backward(const float* weights, const float* ts, const int32_t* rays, const float* nears, const float* fars,
                                       const float* totals, const float* grad_ray, uint32_t M, uint32_t N, int space, int zero_fill,
                                       float* grad_weights, void* stream) {
    N2M_REQUIRE(weights && ts && rays && nears && fars && totals && grad_ray && grad_weights, N2M_ENULL, "distortion_backward: NULL tensor");
    if (int rc = check_distortion("distortion_backward", M, N, space)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (zero_fill) N2M_HIP(hipMemsetAsync(grad_weights, 0, (size_t)M * sizeof(float), s));      // the rows no ray owns
    const uint32_t grid = std::min(n2m_ceil_div(N, 4), kMaxBlocks);
    if (space == N2M_DISTORT_LINEAR)
        distortion_bwd_kernel<0><<<grid, 256, 0, s>>>(weights, ts, rays, nears, fars, totals, grad_ray, M, N, grad_weights);
    else
        distortion_bwd_kernel<1><<<grid, 256, 0, s>>>(weights, ts, rays, nears, fars, totals, grad_ray, M, N, grad_weights);
    N2M_CHECK_LAUNCH();
    return 0;
}
