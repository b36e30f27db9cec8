// The scene contraction of the unbounded recipes (nerf/renderer.py:25-41) on rows of three floats, and the gather that feeds the stage-1
// executor's colour field with it.
//
//   contract:    mag = max(|x|, |y|, |z|);  mag <= 1 ? x : x * (2 - 1 / mag) / mag
//   uncontract:  mag = max(|x|, |y|, |z|);  mag <= 1 ? x : x * (1 / (2 * mag - mag * mag))
//
// Both are the torch statements operation for operation: every product, quotient and difference is rounded on its own (this library is
// built with -ffp-contract=off, and `/` is the correctly rounded division), in the order the statement evaluates them, so the result equals
// the statement's on CPU fp32 tensors bit for bit.  torch.amax hands a NaN on (fmaxf drops it), so a row with a NaN component gets
// mag = NaN, fails `mag <= 1` and comes out all NaN, as in torch; a row with an infinite component goes through the same arithmetic torch
// does (inf / inf = NaN, finite / inf = 0).
#include "n2m_common.hpp"
#include "../../include/n2m_raster.h"

namespace {

__device__ __forceinline__ float amax3(float x, float y, float z) {
    const float m = fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z)));
    return (x != x || y != y || z != z) ? __builtin_nanf("") : m;
}

__device__ __forceinline__ void contract3(float& x, float& y, float& z) {
    const float mag = amax3(x, y, z);
    if (mag <= 1.0f) return;
    const float k = 2.0f - 1.0f / mag;
    x = (x * k) / mag; y = (y * k) / mag; z = (z * k) / mag;
}

__device__ __forceinline__ void uncontract3(float& x, float& y, float& z) {
    const float mag = amax3(x, y, z);
    if (mag <= 1.0f) return;
    const float k = 1.0f / (2.0f * mag - mag * mag);
    x = x * k; y = y * k; z = z * k;
}

// one thread per row; a row is read whole before it is written, so out == xyz is fine
template <bool INVERSE>
__global__ void __launch_bounds__(256)
contract_rows_kernel(const float* xyz, uint32_t N, float* out) {
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= N) return;
    const float* p = xyz + 3 * (size_t)n;
    float x = p[0], y = p[1], z = p[2];
    if (INVERSE) uncontract3(x, y, z); else contract3(x, y, z);
    float* q = out + 3 * (size_t)n;
    q[0] = x; q[1] = y; q[2] = z;
}

// pts[k] = (contracted) img[idx[k], 0:3]; x01[k] = pts[k] mapped from [-bound, bound] to [0, 1].  POW2: 0.5 + pts * (0.5 / bound), the scale
// being exact; else (pts + bound) * (1 / (2 bound)) -- torch's device division by a host scalar multiplies by the reciprocal it forms once.
template <bool POW2>
__global__ void __launch_bounds__(256)
gather_contract_x01_kernel(const float* __restrict__ img, const int64_t* __restrict__ idx, uint32_t K, uint32_t stride, bool vec4, bool contract,
                           float bound, float scale, float* __restrict__ pts, float* __restrict__ x01) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= K) return;
    const float* src = img + (size_t)idx[k] * stride;
    float x, y, z;
    if (vec4) { const float4 v = *reinterpret_cast<const float4*>(src); x = v.x; y = v.y; z = v.z; }
    else { x = src[0]; y = src[1]; z = src[2]; }
    if (contract) contract3(x, y, z);
    float* p = pts + 3 * (size_t)k;
    p[0] = x; p[1] = y; p[2] = z;
    float* u = x01 + 3 * (size_t)k;
    if (POW2) { u[0] = 0.5f + x * scale; u[1] = 0.5f + y * scale; u[2] = 0.5f + z * scale; }
    else { u[0] = (x + bound) * scale; u[1] = (y + bound) * scale; u[2] = (z + bound) * scale; }
}

template <bool INVERSE>
int contract_rows(const char* fn, const float* xyz, uint32_t N, float* out, void* stream) {
    if (N == 0) return 0;
    N2M_REQUIRE(xyz && out, N2M_EINVAL, "%s: NULL tensor with N = %u", fn, N);
    contract_rows_kernel<INVERSE><<<n2m_ceil_div(N, 256), 256, 0, (hipStream_t)stream>>>(xyz, N, out);
    N2M_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int n2m_contract(const float* xyz, uint32_t N, float* out, void* stream) { return contract_rows<false>("n2m_contract", xyz, N, out, stream); }

extern "C" int n2m_uncontract(const float* xyz, uint32_t N, float* out, void* stream) { return contract_rows<true>("n2m_uncontract", xyz, N, out, stream); }

extern "C" int n2m_gather_contract_x01(const float* img, const int64_t* idx, uint32_t K, uint32_t cols_in_stride, int contract, float bound, float* pts,
                                       float* x01, void* stream) {
    if (K == 0) return 0;
    N2M_REQUIRE(img && idx && pts && x01, N2M_EINVAL, "gather_contract_x01: NULL tensor with K = %u", K);
    N2M_REQUIRE(cols_in_stride >= 3, N2M_EINVAL, "gather_contract_x01: a row stride below the row length");
    N2M_REQUIRE(bound > 0.0f && bound < FLT_MAX, N2M_EINVAL, "gather_contract_x01: bound must be positive and finite");
    int e = 0;
    const bool pow2 = frexpf(bound, &e) == 0.5f;
    const bool vec4 = cols_in_stride == 4 && ((uintptr_t)img & 15u) == 0;
    const uint32_t nb = n2m_ceil_div(K, 256);
    hipStream_t s = (hipStream_t)stream;
    if (pow2) gather_contract_x01_kernel<true><<<nb, 256, 0, s>>>(img, idx, K, cols_in_stride, vec4, contract != 0, bound, 0.5f / bound, pts, x01);
    else gather_contract_x01_kernel<false><<<nb, 256, 0, s>>>(img, idx, K, cols_in_stride, vec4, contract != 0, bound, 1.0f / (2.0f * bound), pts, x01);
    N2M_CHECK_LAUNCH();
    return 0;
}
