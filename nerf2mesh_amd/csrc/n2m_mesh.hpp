// Device helpers shared by the mesh passes (meshclean.hip, uvatlas.hip): exact fp64 face frames, the lock-free union-find whose roots
// are their trees' minima, and the order-preserving integer encoding of floats for atomic min / max.
#pragma once
#include "n2m_common.hpp"

namespace {

__device__ __forceinline__ double ldc(const float* __restrict__ v, int32_t i, int c) { return (double)v[3 * (int64_t)i + c]; }

// fp64 cross product (b - a) x (c - a) of face f's fp32 corners: every difference is exact, every product of two differences too
__device__ __forceinline__ void face_cross(const float* __restrict__ verts, const int32_t* __restrict__ faces, uint32_t f, double n[3]) {
    const int32_t a = faces[3 * (int64_t)f], b = faces[3 * (int64_t)f + 1], c = faces[3 * (int64_t)f + 2];
    const double ux = ldc(verts, b, 0) - ldc(verts, a, 0), uy = ldc(verts, b, 1) - ldc(verts, a, 1), uz = ldc(verts, b, 2) - ldc(verts, a, 2);
    const double wx = ldc(verts, c, 0) - ldc(verts, a, 0), wy = ldc(verts, c, 1) - ldc(verts, a, 1), wz = ldc(verts, c, 2) - ldc(verts, a, 2);
    n[0] = uy * wz - uz * wy;
    n[1] = uz * wx - ux * wz;
    n[2] = ux * wy - uy * wx;
}

__device__ __forceinline__ int32_t uf_load(int32_t* parent, int32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x with path halving: a non-root's parent only ever moves to an ancestor, so a stale halving write is harmless
__device__ __forceinline__ int32_t uf_find(int32_t* parent, int32_t x) {
    int32_t p = uf_load(parent, x);
    while (p != x) {
        const int32_t g = uf_load(parent, p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

// the larger root is always hooked under the smaller one: every root is its tree's minimum, whatever order the hooks ran in
__device__ __forceinline__ void uf_unite(int32_t* parent, int32_t a, int32_t b) {
    while (true) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a > b) { const int32_t x = a; a = b; b = x; }
        int32_t expected = b;
        if (__hip_atomic_compare_exchange_strong(parent + b, &expected, a, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    }
}

// order-preserving u32 encoding of a float (monotone in the float's value; -0 below +0), and its inverse: flip every bit of a negative
// float, only the sign bit of a positive one.  (The inverse is written without a select: the select form crashes this compiler's
// instruction selection.)
__device__ __forceinline__ uint32_t fenc(float x) {
    const uint32_t b = __float_as_uint(x);
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float fdec(uint32_t e) { return __uint_as_float(e ^ (~(uint32_t)((int32_t)e >> 31) | 0x80000000u)); }

}  // namespace
