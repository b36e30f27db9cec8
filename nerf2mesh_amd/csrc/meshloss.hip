// The two mesh losses of stage 1 that the reference takes from pytorch3d (nerf/utils.py:759-769: mesh_normal_consistency, mesh_edge_loss), on
// the topology trainer.MeshEdgeTerms builds once per mesh:
//
//   edges [E, 2] int32  unique undirected edges, v0 < v1
//   pairs [P, 4] int32  (v0, v1, a, b): for an edge with k incident faces one record per pair of faces (k (k - 1) / 2 of them), v0 < v1 the
//                       edge's endpoints, a / b the vertices opposite the edge in the first / second face
//
// normal consistency: e = v1 - v0, n0 = e x (a - v0), n1 = -(e x (b - v0)), c = n0 . n1 / (max(|n0|, 1e-8) max(|n1|, 1e-8))
// (torch.cosine_similarity, default eps), term 1 - c; edge length (target 0): term |v0 - v1|^2.  The caller folds the means (1 / P, 1 / E)
// and the loss weights into w_normal / w_edge.
//
// forward: one thread per pair, then one thread per edge; per-workgroup sums in a fixed order (no atomics).
// backward: GATHER form -- one thread per vertex walks its two CSR rows (vertex -> the terms it takes part in, ascending) and recomputes the
// gradient of each incident term for its own corner: a fixed summation order, so the gradient is the same bits on every run.
// Entry points are declared in include/n2m_raster.h.
#include "n2m_common.hpp"

namespace {

constexpr float kCosEps = 1e-8f;      // torch.cosine_similarity's default eps

struct V3 {
    float x, y, z;
};

__device__ __forceinline__ V3 ld3(const float* __restrict__ v, int32_t i) {
    const size_t j = (size_t)i * 3u;
    return {v[j], v[j + 1], v[j + 2]};
}
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 mul(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 div(V3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// One pair's geometry: the two face normals (n1 already carries its minus sign: -(e x q) = q x e), their norms and clamped norms.
struct PairGeo {
    V3 e, p, q, n0, n1;
    float l0, l1, d0, d1;
};

__device__ __forceinline__ PairGeo pair_geo(const float* __restrict__ v, int4 r) {
    PairGeo g;
    const V3 v0 = ld3(v, r.x);
    g.e = sub(ld3(v, r.y), v0);
    g.p = sub(ld3(v, r.z), v0);
    g.q = sub(ld3(v, r.w), v0);
    g.n0 = cross(g.e, g.p);
    g.n1 = cross(g.q, g.e);
    g.l0 = sqrtf(dot(g.n0, g.n0));
    g.l1 = sqrtf(dot(g.n1, g.n1));
    g.d0 = fmaxf(g.l0, kCosEps);
    g.d1 = fmaxf(g.l1, kCosEps);
    return g;
}

// c = (n0 / d0) . (n1 / d1): each normal divided by its own clamped norm first, as torch does (a product of two tiny norms would underflow)
__device__ __forceinline__ float pair_cos(const PairGeo& g) { return dot(div(g.n0, g.d0), div(g.n1, g.d1)); }

// d (1 - c) / d (corner k of the pair), k = 0..3 for v0, v1, a, b.  With u0 = n0 / d0, u1 = n1 / d1:
//   dc / dn0 = (u1 - [l0 >= eps] (u0 . u1) u0) / d0   (below eps the norm is clamped to a constant: only the first part is left, and it is
//   finite for a zero-area face), the same for n1; n0 = e x p, n1 = q x e give
//   dc / de = p x g0 + g1 x q,  dc / dp = g0 x e,  dc / dq = e x g1,  and v0 takes minus their sum.
__device__ __forceinline__ V3 pair_grad(const PairGeo& g, uint32_t k) {
    const V3 u0 = div(g.n0, g.d0), u1 = div(g.n1, g.d1);
    const float c = dot(u0, u1);
    const V3 g0 = div(sub(u1, mul(u0, g.l0 >= kCosEps ? c : 0.0f)), g.d0);
    const V3 g1 = div(sub(u0, mul(u1, g.l1 >= kCosEps ? c : 0.0f)), g.d1);
    const V3 ge = add(cross(g.p, g0), cross(g1, g.q));
    const V3 gp = cross(g0, g.e);
    const V3 gq = cross(g.e, g1);
    V3 d;                                                     // dc / d corner
    if (k == 0u) d = mul(add(add(ge, gp), gq), -1.0f);
    else if (k == 1u) d = ge;
    else if (k == 2u) d = gp;
    else d = gq;
    return mul(d, -1.0f);                                     // the term is 1 - c
}

// blocks [0, nbp): pairs; blocks [nbp, nbp + nbe): edges.  partial[block] = the workgroup's sum, waves in a fixed order.
__global__ void __launch_bounds__(256)
mesh_losses_forward_kernel(const float* __restrict__ v, const int32_t* __restrict__ pairs, uint32_t P, const int32_t* __restrict__ edges, uint32_t E,
                           uint32_t nbp, float w_normal, float w_edge, float* __restrict__ partial) {
    __shared__ float red[4];
    float term = 0.0f;
    if (blockIdx.x < nbp) {
        const uint32_t t = blockIdx.x * 256u + threadIdx.x;
        if (t < P) {
            const PairGeo g = pair_geo(v, *reinterpret_cast<const int4*>(pairs + (size_t)t * 4u));
            term = (1.0f - pair_cos(g)) * w_normal;
        }
    } else {
        const uint32_t t = (blockIdx.x - nbp) * 256u + threadIdx.x;
        if (t < E) {
            const int2 r = *reinterpret_cast<const int2*>(edges + (size_t)t * 2u);
            const V3 d = sub(ld3(v, r.x), ld3(v, r.y));
            term = dot(d, d) * w_edge;
        }
    }
    const float w = n2m_wave_sum(term);
    if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0u) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// pair_ref[k] = 4 * pair + corner, edge_ref[k] = 2 * edge + corner; a row's entries ascend.
template <bool ACC>
__global__ void __launch_bounds__(256)
mesh_losses_backward_kernel(const float* __restrict__ v, const int32_t* __restrict__ pairs, const int32_t* __restrict__ pair_ptr,
                            const int32_t* __restrict__ pair_ref, const int32_t* __restrict__ edges, const int32_t* __restrict__ edge_ptr,
                            const int32_t* __restrict__ edge_ref, uint32_t V, const float* __restrict__ grad, float w_normal, float w_edge,
                            float* __restrict__ d_v) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= V) return;
    V3 sn = {0.f, 0.f, 0.f}, se = {0.f, 0.f, 0.f};
    if (pair_ptr) {
        for (int32_t k = pair_ptr[i], end = pair_ptr[i + 1]; k < end; ++k) {
            const uint32_t ref = (uint32_t)pair_ref[k];
            const PairGeo g = pair_geo(v, *reinterpret_cast<const int4*>(pairs + (size_t)(ref >> 2) * 4u));
            sn = add(sn, pair_grad(g, ref & 3u));
        }
    }
    if (edge_ptr) {
        const V3 vi = ld3(v, (int32_t)i);
        for (int32_t k = edge_ptr[i], end = edge_ptr[i + 1]; k < end; ++k) {
            const uint32_t ref = (uint32_t)edge_ref[k];
            se = add(se, sub(vi, ld3(v, edges[(size_t)(ref ^ 1u)])));      // d |v0 - v1|^2 / d (this end) = 2 (this end - the other end)
        }
    }
    const float gs = *grad;
    const V3 t = add(mul(sn, gs * w_normal), mul(se, gs * w_edge * 2.0f));
    float* o = d_v + (size_t)i * 3u;
    if (ACC) { o[0] += t.x; o[1] += t.y; o[2] += t.z; }
    else { o[0] = t.x; o[1] = t.y; o[2] = t.z; }
}

int check_backward(const float* verts, const int32_t* pairs, const int32_t* pair_ptr, const int32_t* pair_ref, uint32_t P, const int32_t* edges,
                   const int32_t* edge_ptr, const int32_t* edge_ref, uint32_t E, const float* grad, float* d_verts) {
    N2M_REQUIRE(verts && grad && d_verts, N2M_ENULL, "mesh_losses_backward: NULL tensor");
    N2M_REQUIRE(P == 0 || (pairs && pair_ptr && pair_ref), N2M_ENULL, "mesh_losses_backward: P > 0 needs pairs, pair_ptr and pair_ref");
    N2M_REQUIRE(E == 0 || (edges && edge_ptr && edge_ref), N2M_ENULL, "mesh_losses_backward: E > 0 needs edges, edge_ptr and edge_ref");
    N2M_REQUIRE(P < (1u << 29) && E < (1u << 30), N2M_EINVAL, "mesh_losses_backward: too many terms for the packed (term, corner) references");
    N2M_REQUIRE(P == 0 || ((uintptr_t)pairs & 15u) == 0, N2M_EINVAL, "mesh_losses_backward: pairs must be 16-byte aligned");
    return 0;
}

}  // namespace

extern "C" int n2m_mesh_losses_forward(const float* verts, const int32_t* pairs, uint32_t P, const int32_t* edges, uint32_t E, float w_normal,
                                       float w_edge, float* partial, void* stream) {
    if (P == 0 && E == 0) return 0;
    N2M_REQUIRE(verts && partial, N2M_ENULL, "mesh_losses_forward: NULL tensor");
    N2M_REQUIRE(P == 0 || pairs, N2M_ENULL, "mesh_losses_forward: P > 0 needs pairs");
    N2M_REQUIRE(E == 0 || edges, N2M_ENULL, "mesh_losses_forward: E > 0 needs edges");
    N2M_REQUIRE(P == 0 || ((uintptr_t)pairs & 15u) == 0, N2M_EINVAL, "mesh_losses_forward: pairs must be 16-byte aligned");
    N2M_REQUIRE(E == 0 || ((uintptr_t)edges & 7u) == 0, N2M_EINVAL, "mesh_losses_forward: edges must be 8-byte aligned");
    const uint32_t nbp = n2m_ceil_div(P, 256), nbe = n2m_ceil_div(E, 256);
    mesh_losses_forward_kernel<<<nbp + nbe, 256, 0, (hipStream_t)stream>>>(verts, pairs, P, edges, E, nbp, w_normal, w_edge, partial);
    N2M_CHECK_LAUNCH();
    return 0;
}

extern "C" int n2m_mesh_losses_backward(const float* verts, const int32_t* pairs, const int32_t* pair_ptr, const int32_t* pair_ref, uint32_t P,
                                        const int32_t* edges, const int32_t* edge_ptr, const int32_t* edge_ref, uint32_t E, uint32_t V,
                                        const float* grad, float w_normal, float w_edge, float* d_verts, void* stream) {
    if (V == 0 || (P == 0 && E == 0)) return 0;
    if (int rc = check_backward(verts, pairs, pair_ptr, pair_ref, P, edges, edge_ptr, edge_ref, E, grad, d_verts)) return rc;
    mesh_losses_backward_kernel<false><<<n2m_ceil_div(V, 256), 256, 0, (hipStream_t)stream>>>(
        verts, pairs, P ? pair_ptr : nullptr, pair_ref, edges, E ? edge_ptr : nullptr, edge_ref, V, grad, w_normal, w_edge, d_verts);
    N2M_CHECK_LAUNCH();
    return 0;
}

extern "C" int n2m_mesh_losses_backward_acc(const float* verts, const int32_t* pairs, const int32_t* pair_ptr, const int32_t* pair_ref, uint32_t P,
                                            const int32_t* edges, const int32_t* edge_ptr, const int32_t* edge_ref, uint32_t E, uint32_t V,
                                            const float* grad, float w_normal, float w_edge, float* d_verts, void* stream) {
    if (V == 0 || (P == 0 && E == 0)) return 0;
    if (int rc = check_backward(verts, pairs, pair_ptr, pair_ref, P, edges, edge_ptr, edge_ref, E, grad, d_verts)) return rc;
    mesh_losses_backward_kernel<true><<<n2m_ceil_div(V, 256), 256, 0, (hipStream_t)stream>>>(
        verts, pairs, P ? pair_ptr : nullptr, pair_ref, edges, E ? edge_ptr : nullptr, edge_ref, V, grad, w_normal, w_edge, d_verts);
    N2M_CHECK_LAUNCH();
    return 0;
}
