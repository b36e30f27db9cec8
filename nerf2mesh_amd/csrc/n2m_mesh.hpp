// Device helpers shared by the mesh passes (meshclean.hip, uvatlas.hip, meshremesh.hip, meshquery.hip): exact fp64 face frames, the
// lock-free union-find whose roots are their trees' minima, the order-preserving integer encoding of floats for atomic min / max, and
// the fp64 closest point of a triangle.
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

// fp64 points: every value a mesh pass decides on is fp64 + - * / (IEEE correctly rounded, -ffp-contract=off)
struct D3 { double x, y, z; };
__device__ __forceinline__ D3 add(D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 sub(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 mul(D3 a, double s) { return D3{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// closest point of the triangle (a, b, c) to p: the Voronoi-region walk (vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, inside)
__device__ __forceinline__ D3 closest_on_triangle(D3 p, D3 a, D3 b, D3 c) {
    const D3 ab = sub(b, a), ac = sub(c, a), ap = sub(p, a);
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) return a;
    const D3 bp = sub(p, b);
    const double d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) return b;
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) return add(a, mul(ab, d1 / (d1 - d3)));
    const D3 cp = sub(p, c);
    const double d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) return c;
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) return add(a, mul(ac, d2 / (d2 - d6)));
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) return add(b, mul(sub(c, b), (d4 - d3) / ((d4 - d3) + (d5 - d6))));
    const double s = (va + vb) + vc;
    return add(add(a, mul(ab, vb / s)), mul(ac, vc / s));
}

}  // namespace
