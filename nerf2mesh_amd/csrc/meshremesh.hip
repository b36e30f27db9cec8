// Isotropic explicit re-meshing on the device (Botsch & Kobbelt 2004: split long edges, collapse short edges, flip towards regular
// valence, relax tangentially): what the reference does on the host with pymeshlab's `meshing_isotropic_explicit_remeshing`
// (meshutils.py:208-209).  The passes below are the per-element work that csrc/meshsimplify.hip does not already have; the rounds, the
// edge / CSR plumbing and the reuse of the 4.11 entry points (selection, collapse, compaction, subdivision emitters) are in
// nerf2mesh_amd/mesh_remesh.py.  DESIGN.md section 4.14 states the rule; tests/mesh_remesh_ref.py restates it in numpy, bit for bit.
//
// Mesh layout as in meshsimplify.hip.  In addition: ecorn [3F] i32 = the corner ids (3 f + k) sorted by the id of the edge the corner
// owns (stable, so ascending face id within an edge), eoff [E + 1] i32 its offsets: the faces of edge e are ecorn[eoff[e] .. eoff[e+1]).
//
// Every value a decision depends on is fp64 + - * / and sqrt (IEEE correctly rounded, -ffp-contract=off), positions are rounded to fp32
// once when stored, and the only atomics are integer min / or / add, whose results do not depend on their order.
#include <math.h>

#include "n2m_common.hpp"
#include "n2m_mesh.hpp"

namespace {

constexpr uint32_t kRmBlock = 256;
constexpr uint32_t kFrozen = 1u, kBoundary = 2u, kFeature = 4u;     // vertex classes (kFrozen, kBoundary: the bits of n2m_mesh_vertex_flags)
constexpr uint64_t kNoKey = ~0ull;
constexpr int64_t kMaxGain = 1ll << 30;

__device__ __forceinline__ D3 ld3(const float* __restrict__ v, int32_t i) {
    return D3{(double)v[3 * (int64_t)i], (double)v[3 * (int64_t)i + 1], (double)v[3 * (int64_t)i + 2]};
}
__device__ __forceinline__ void st3(float* __restrict__ v, int32_t i, D3 p) {
    v[3 * (int64_t)i] = (float)p.x; v[3 * (int64_t)i + 1] = (float)p.y; v[3 * (int64_t)i + 2] = (float)p.z;
}
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ D3 round_f32(D3 p) { return D3{(double)(float)p.x, (double)(float)p.y, (double)(float)p.z}; }
__device__ __forceinline__ D3 face_normal(const float* __restrict__ verts, const int32_t* __restrict__ t) {
    const D3 p0 = ld3(verts, t[0]);
    return cross(sub(ld3(verts, t[1]), p0), sub(ld3(verts, t[2]), p0));
}
__device__ __forceinline__ int32_t other_end(const int32_t* __restrict__ edges, int32_t e, int32_t v) {
    return edges[2 * (int64_t)e] ^ edges[2 * (int64_t)e + 1] ^ v;
}

// the tie-break of 4.11's keys (murmur3's finaliser, a bijection of the 32-bit edge id)
__device__ __forceinline__ uint32_t mix_id(uint32_t h) {
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

// ------------------------------------------------------------------------------------------------------------ split mark
__global__ void rm_split_long_kernel(const float* __restrict__ verts, const int32_t* __restrict__ edges, uint32_t E, double thr2,
                                     uint8_t* __restrict__ split) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const D3 d = sub(ld3(verts, edges[2 * (int64_t)e + 1]), ld3(verts, edges[2 * (int64_t)e]));
    split[e] = dot(d, d) > thr2 ? 1 : 0;
}

// an edge with an unselected face is not split (every writer stores 0: no order to depend on)
__global__ void rm_split_unselected_kernel(uint32_t F, const int32_t* __restrict__ c2e, const uint8_t* __restrict__ face_sel,
                                           uint8_t* __restrict__ split) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F || face_sel[f]) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) split[c2e[3 * (int64_t)f + k]] = 0;
}

// ------------------------------------------------------------------------------------------------------------ features
__global__ void rm_edge_feature_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, uint32_t E,
                                       const int32_t* __restrict__ eoff, const int32_t* __restrict__ ecorn, double cos_feature,
                                       uint8_t* __restrict__ efeat) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int32_t o = eoff[e];
    if (eoff[e + 1] - o != 2) { efeat[e] = 1; return; }
    const D3 n0 = face_normal(verts, faces + 3 * (int64_t)(ecorn[o] / 3)), n1 = face_normal(verts, faces + 3 * (int64_t)(ecorn[o + 1] / 3));
    efeat[e] = dot(n0, n1) < cos_feature * (sqrt(dot(n0, n0)) * sqrt(dot(n1, n1))) ? 1 : 0;
}

// vclass = flags | kFeature (two feature edges that go on straight within the feature angle: the vertex may slide along them)
//                | kFrozen  (one feature edge, more than two, or two that turn by more than the feature angle: a corner)
__global__ void rm_vertex_class_kernel(const float* __restrict__ verts, const int32_t* __restrict__ edges, const int32_t* __restrict__ ve_off,
                                       const int32_t* __restrict__ ve_idx, uint32_t V, const uint8_t* __restrict__ efeat,
                                       const uint32_t* __restrict__ flags, double cos_feature, uint32_t* __restrict__ vclass) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    int n = 0;
    int32_t w[2] = {0, 0};
    for (int32_t j = ve_off[v]; j < ve_off[v + 1]; ++j) {
        const int32_t e = ve_idx[j];
        if (!efeat[e]) continue;
        if (n < 2) w[n] = other_end(edges, e, (int32_t)v);
        ++n;
    }
    uint32_t c = flags[v];
    if (n == 2) {
        const D3 p = ld3(verts, (int32_t)v);
        const D3 d1 = sub(ld3(verts, w[0]), p), d2 = sub(ld3(verts, w[1]), p);
        const bool corner = dot(d1, d2) > -cos_feature * (sqrt(dot(d1, d1)) * sqrt(dot(d2, d2)));
        c |= corner ? kFrozen : kFeature;
    } else if (n != 0) {
        c |= kFrozen;
    }
    vclass[v] = c;
}

// ------------------------------------------------------------------------------------------------------------ collapse cost
// the sum of the cross products of the faces of v, in ascending face id: the area-weighted vertex normal, not normalised
__device__ __forceinline__ D3 star_normal(const float* __restrict__ verts, const int32_t* __restrict__ faces, const int32_t* __restrict__ vf_off,
                                          const int32_t* __restrict__ vf_idx, int32_t v) {
    D3 n = D3{0.0, 0.0, 0.0};
    for (int32_t j = vf_off[v]; j < vf_off[v + 1]; ++j) n = add(n, face_normal(verts, faces + 3 * (int64_t)vf_idx[j]));
    return n;
}

// a face around v that survives the collapse of (a, b) into p must keep a positive dot product with its old normal (4.11's test) and
// with the old vertex normal of v: a sliver's own normal turns by almost 90 degrees per operation, the vertex normal does not follow it
__device__ __forceinline__ bool star_flips(const float* __restrict__ verts, const int32_t* __restrict__ faces, const int32_t* __restrict__ vf_off,
                                           const int32_t* __restrict__ vf_idx, int32_t v, int32_t a, int32_t b, D3 p) {
    const D3 nv = star_normal(verts, faces, vf_off, vf_idx, v);
    for (int32_t j = vf_off[v]; j < vf_off[v + 1]; ++j) {
        const int32_t* t = faces + 3 * (int64_t)vf_idx[j];
        const bool has_a = t[0] == a || t[1] == a || t[2] == a, has_b = t[0] == b || t[1] == b || t[2] == b;
        if (has_a && has_b) continue;
        D3 o[3], w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = ld3(verts, t[k]);
            w[k] = (t[k] == a || t[k] == b) ? p : o[k];
        }
        const D3 n0 = cross(sub(o[1], o[0]), sub(o[2], o[0]));
        const D3 n1 = cross(sub(w[1], w[0]), sub(w[2], w[0]));
        if (!(dot(n1, n0) > 0.0 && dot(n1, nv) > 0.0)) return true;
    }
    return false;
}

// an edge from p to a neighbour of v (other than a, b) longer than hi
__device__ __forceinline__ bool makes_long_edge(const float* __restrict__ verts, const int32_t* __restrict__ edges, const int32_t* __restrict__ ve_off,
                                                const int32_t* __restrict__ ve_idx, int32_t v, int32_t a, int32_t b, D3 p, double hi2) {
    for (int32_t j = ve_off[v]; j < ve_off[v + 1]; ++j) {
        const int32_t w = other_end(edges, ve_idx[j], v);
        if (w == a || w == b) continue;
        const D3 d = sub(ld3(verts, w), p);
        if (dot(d, d) > hi2) return true;
    }
    return false;
}

__global__ void rm_collapse_cost_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, const int32_t* __restrict__ edges,
                                        const int32_t* __restrict__ nf, uint32_t E, const uint32_t* __restrict__ vclass,
                                        const uint8_t* __restrict__ efeat, const int32_t* __restrict__ vf_off, const int32_t* __restrict__ vf_idx,
                                        const int32_t* __restrict__ ve_off, const int32_t* __restrict__ ve_idx, double lo2, double hi2,
                                        uint64_t* __restrict__ keys, float* __restrict__ placement) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    keys[e] = kNoKey;
    const int32_t a = edges[2 * (int64_t)e], b = edges[2 * (int64_t)e + 1];
    const D3 pa = ld3(verts, a), pb = ld3(verts, b);
    const D3 ab = sub(pb, pa);
    const double len2 = dot(ab, ab);
    if (!(len2 < lo2)) return;
    const int32_t n = nf[e];
    const uint32_t ca = vclass[a], cb = vclass[b];
    if (n > 2 || ((ca | cb) & kFrozen)) return;
    const bool fa = (ca & kFeature) != 0, fb = (cb & kFeature) != 0;
    if (fa && fb && !efeat[e]) return;                          // two feature (or boundary) vertices: only along the feature
    int32_t common = 0;                                         // link condition: common neighbours == faces on the edge
    {
        int32_t i = ve_off[a], j = ve_off[b];
        const int32_t ie = ve_off[a + 1], je = ve_off[b + 1];
        while (i < ie && j < je) {
            const int32_t na = other_end(edges, ve_idx[i], a), nb = other_end(edges, ve_idx[j], b);
            if (na == nb) { ++common; ++i; ++j; }
            else if (na < nb) ++i;
            else ++j;
        }
    }
    if (common != n) return;
    D3 p;
    if (fa == fb) p = round_f32(D3{(pa.x + pb.x) * 0.5, (pa.y + pb.y) * 0.5, (pa.z + pb.z) * 0.5});
    else p = fa ? pa : pb;
    if (star_flips(verts, faces, vf_off, vf_idx, a, a, b, p) || star_flips(verts, faces, vf_off, vf_idx, b, a, b, p)) return;
    if (makes_long_edge(verts, edges, ve_off, ve_idx, a, a, b, p, hi2) || makes_long_edge(verts, edges, ve_off, ve_idx, b, a, b, p, hi2)) return;
    keys[e] = ((uint64_t)__float_as_uint((float)len2) << 32) | (uint64_t)mix_id(e);
    st3(placement, (int32_t)e, p);
}

// ------------------------------------------------------------------------------------------------------------ flips
__device__ __forceinline__ int64_t valence_dev(const int32_t* __restrict__ ve_off, const uint32_t* __restrict__ vclass, int32_t v, int delta) {
    const int64_t d = (int64_t)(ve_off[v + 1] - ve_off[v]) + delta - ((vclass[v] & kBoundary) ? 4 : 6);
    return d * d;
}

// quad [E][6] = x, y, c, d, f0, f1: f0 = (x, y, c) and f1 = (y, x, d) up to rotation become (c, x, d) and (d, y, c)
__global__ void rm_flip_candidates_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, const uint8_t* __restrict__ face_sel,
                                          const int32_t* __restrict__ edges, uint32_t E, const int32_t* __restrict__ eoff,
                                          const int32_t* __restrict__ ecorn, const uint8_t* __restrict__ efeat, const uint32_t* __restrict__ vclass,
                                          const int32_t* __restrict__ ve_off, const int32_t* __restrict__ ve_idx, uint64_t* __restrict__ keys,
                                          int32_t* __restrict__ quad, unsigned long long* __restrict__ m1) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    keys[e] = kNoKey;
    const int32_t o = eoff[e];
    if (eoff[e + 1] - o != 2 || efeat[e]) return;
    const int32_t c0 = ecorn[o], c1 = ecorn[o + 1];
    const int32_t f0 = c0 / 3, k0 = c0 % 3, f1 = c1 / 3, k1 = c1 % 3;
    if (!face_sel[f0] || !face_sel[f1]) return;
    const int32_t* t0 = faces + 3 * (int64_t)f0;
    const int32_t* t1 = faces + 3 * (int64_t)f1;
    const int32_t x = t0[k0], y = t0[(k0 + 1) % 3], c = t0[(k0 + 2) % 3], d = t1[(k1 + 2) % 3];
    if (t1[k1] != y || t1[(k1 + 1) % 3] != x || c == d) return;      // the two faces must run through the edge in opposite directions
    for (int32_t j = ve_off[c]; j < ve_off[c + 1]; ++j)
        if (other_end(edges, ve_idx[j], c) == d) return;             // (c, d) is an edge already
    const int64_t gain = valence_dev(ve_off, vclass, x, 0) + valence_dev(ve_off, vclass, y, 0) + valence_dev(ve_off, vclass, c, 0) +
                         valence_dev(ve_off, vclass, d, 0) - valence_dev(ve_off, vclass, x, -1) - valence_dev(ve_off, vclass, y, -1) -
                         valence_dev(ve_off, vclass, c, 1) - valence_dev(ve_off, vclass, d, 1);
    if (gain <= 0) return;
    const D3 px = ld3(verts, x), py = ld3(verts, y), pc = ld3(verts, c), pd = ld3(verts, d);
    const D3 n0 = cross(sub(py, px), sub(pc, px)), n1 = cross(sub(px, py), sub(pd, py));
    const D3 g0 = cross(sub(px, pc), sub(pd, pc)), g1 = cross(sub(py, pd), sub(pc, pd));
    if (!(dot(g0, n0) > 0.0 && dot(g0, n1) > 0.0 && dot(g1, n0) > 0.0 && dot(g1, n1) > 0.0)) return;
    const int64_t g = gain < kMaxGain ? gain : kMaxGain;
    const uint64_t key = ((uint64_t)(kMaxGain - g) << 32) | (uint64_t)mix_id(e);
    keys[e] = key;
    int32_t* q = quad + 6 * (int64_t)e;
    q[0] = x; q[1] = y; q[2] = c; q[3] = d; q[4] = f0; q[5] = f1;
    atomicMin(m1 + x, (unsigned long long)key); atomicMin(m1 + y, (unsigned long long)key);
    atomicMin(m1 + c, (unsigned long long)key); atomicMin(m1 + d, (unsigned long long)key);
}

// selected: the key is the minimum at all four vertices, so the selected quadruples are pairwise disjoint (and so are their faces)
__global__ void rm_flip_apply_kernel(uint32_t E, const uint64_t* __restrict__ keys, const int32_t* __restrict__ quad,
                                     const unsigned long long* __restrict__ m1, int32_t* __restrict__ faces, int32_t* __restrict__ face_src,
                                     unsigned long long* __restrict__ total) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const uint64_t k = keys[e];
    if (k == kNoKey) return;
    const int32_t* q = quad + 6 * (int64_t)e;
    const int32_t x = q[0], y = q[1], c = q[2], d = q[3], f0 = q[4], f1 = q[5];
    if (m1[x] != k || m1[y] != k || m1[c] != k || m1[d] != k) return;
    int32_t* t0 = faces + 3 * (int64_t)f0;
    int32_t* t1 = faces + 3 * (int64_t)f1;
    t0[0] = c; t0[1] = x; t0[2] = d;
    t1[0] = d; t1[1] = y; t1[2] = c;
    const int32_t s0 = face_src[f0], s1 = face_src[f1];
    face_src[f0] = face_src[f1] = s0 < s1 ? s0 : s1;
    atomicAdd(total, 1ull);
}

// ------------------------------------------------------------------------------------------------------------ relax
// (closest_on_triangle, the Voronoi-region walk, is in n2m_mesh.hpp: csrc/meshquery.hip shares it)
__global__ void rm_relax_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, const int32_t* __restrict__ edges,
                                const uint32_t* __restrict__ vclass, const int32_t* __restrict__ vf_off, const int32_t* __restrict__ vf_idx,
                                const int32_t* __restrict__ ve_off, const int32_t* __restrict__ ve_idx, uint32_t V, float* __restrict__ out,
                                uint8_t* __restrict__ moved, double* __restrict__ vnormal) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    moved[v] = 0;
    const int32_t deg = ve_off[v + 1] - ve_off[v];
    if (vclass[v] != 0u || deg == 0) return;
    const D3 p = ld3(verts, (int32_t)v);
    D3 q = D3{0.0, 0.0, 0.0};
    for (int32_t j = ve_off[v]; j < ve_off[v + 1]; ++j) q = add(q, ld3(verts, other_end(edges, ve_idx[j], (int32_t)v)));
    q = D3{q.x / (double)deg, q.y / (double)deg, q.z / (double)deg};
    const D3 n = star_normal(verts, faces, vf_off, vf_idx, (int32_t)v);
    const double nn = dot(n, n);
    if (!(nn > 0.0)) return;
    const double t = dot(n, sub(p, q)) / nn;
    const D3 r = add(q, mul(n, t));                             // the mean of the neighbours, brought back into the tangent plane at p
    double best = INFINITY;
    D3 hit = p;
    for (int32_t j = vf_off[v]; j < vf_off[v + 1]; ++j) {
        const int32_t* tr = faces + 3 * (int64_t)vf_idx[j];
        const D3 c = closest_on_triangle(r, ld3(verts, tr[0]), ld3(verts, tr[1]), ld3(verts, tr[2]));
        const D3 d = sub(c, r);
        const double dd = dot(d, d);
        if (dd < best) { best = dd; hit = c; }
    }
    if (!(best < INFINITY)) return;
    st3(out, (int32_t)v, hit);
    moved[v] = 1;
    vnormal[3 * (int64_t)v] = n.x; vnormal[3 * (int64_t)v + 1] = n.y; vnormal[3 * (int64_t)v + 2] = n.z;
}

__global__ void rm_relax_offending_kernel(const float* __restrict__ before, const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                          uint32_t F, const uint8_t* __restrict__ moved, const double* __restrict__ vnormal,
                                          uint8_t* __restrict__ revert) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int32_t* t = faces + 3 * (int64_t)f;
    if (!(moved[t[0]] | moved[t[1]] | moved[t[2]])) return;
    const D3 g = face_normal(verts, t);
    bool ok = dot(g, face_normal(before, t)) > 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k)                                 // and with the old vertex normal of every corner that moved
        if (moved[t[k]]) ok = ok && dot(g, D3{vnormal[3 * (int64_t)t[k]], vnormal[3 * (int64_t)t[k] + 1], vnormal[3 * (int64_t)t[k] + 2]}) > 0.0;
    if (ok) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) revert[t[k]] = 1;
}

__global__ void rm_relax_revert_kernel(const float* __restrict__ before, float* __restrict__ verts, uint32_t V, uint8_t* __restrict__ moved,
                                       const uint8_t* __restrict__ revert, unsigned long long* __restrict__ total) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V || !revert[v] || !moved[v]) return;
#pragma unroll
    for (int i = 0; i < 3; ++i) verts[3 * (int64_t)v + i] = before[3 * (int64_t)v + i];
    moved[v] = 0;
    atomicAdd(total, 1ull);
}

inline uint32_t grid_of(uint64_t n) { return n2m_ceil_div(n, kRmBlock); }

}  // namespace

extern "C" {

int n2m_mesh_remesh_split_mark(const float* vertices, const int32_t* edges, uint32_t E, uint32_t F, const int32_t* c2e, const uint8_t* face_sel,
                               double threshold_sq, uint8_t* split, void* stream) {
    if (E == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(edges); N2M_NOTNULL(c2e); N2M_NOTNULL(face_sel); N2M_NOTNULL(split);
    hipStream_t s = (hipStream_t)stream;
    rm_split_long_kernel<<<grid_of(E), kRmBlock, 0, s>>>(vertices, edges, E, threshold_sq, split);
    N2M_CHECK_LAUNCH();
    if (F == 0) return 0;
    rm_split_unselected_kernel<<<grid_of(F), kRmBlock, 0, s>>>(F, c2e, face_sel, split);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_remesh_classify(const float* vertices, uint32_t V, const int32_t* faces, const int32_t* edges, uint32_t E, const int32_t* edge_offsets,
                             const int32_t* edge_corners, const int32_t* ve_offsets, const int32_t* ve_edges, const uint32_t* flags,
                             double cos_feature, uint8_t* edge_feature, uint32_t* vertex_class, void* stream) {
    if (V == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(ve_offsets); N2M_NOTNULL(flags); N2M_NOTNULL(vertex_class);
    hipStream_t s = (hipStream_t)stream;
    if (E) {
        N2M_NOTNULL(faces); N2M_NOTNULL(edges); N2M_NOTNULL(edge_offsets); N2M_NOTNULL(edge_corners); N2M_NOTNULL(ve_edges); N2M_NOTNULL(edge_feature);
        rm_edge_feature_kernel<<<grid_of(E), kRmBlock, 0, s>>>(vertices, faces, E, edge_offsets, edge_corners, cos_feature, edge_feature);
        N2M_CHECK_LAUNCH();
    }
    rm_vertex_class_kernel<<<grid_of(V), kRmBlock, 0, s>>>(vertices, edges, ve_offsets, ve_edges, V, edge_feature, flags, cos_feature, vertex_class);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_remesh_collapse_cost(const float* vertices, const int32_t* faces, const int32_t* edges, const int32_t* edge_nf, uint32_t E,
                                  const uint32_t* vertex_class, const uint8_t* edge_feature, const int32_t* vf_offsets, const int32_t* vf_faces,
                                  const int32_t* ve_offsets, const int32_t* ve_edges, double lo_sq, double hi_sq, uint64_t* keys, float* placement,
                                  void* stream) {
    if (E == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(faces); N2M_NOTNULL(edges); N2M_NOTNULL(edge_nf); N2M_NOTNULL(vertex_class); N2M_NOTNULL(edge_feature);
    N2M_NOTNULL(vf_offsets); N2M_NOTNULL(vf_faces); N2M_NOTNULL(ve_offsets); N2M_NOTNULL(ve_edges); N2M_NOTNULL(keys); N2M_NOTNULL(placement);
    rm_collapse_cost_kernel<<<grid_of(E), kRmBlock, 0, (hipStream_t)stream>>>(vertices, faces, edges, edge_nf, E, vertex_class, edge_feature,
                                                                            vf_offsets, vf_faces, ve_offsets, ve_edges, lo_sq, hi_sq, keys, placement);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_remesh_flip_round(const float* vertices, uint32_t V, int32_t* faces, const uint8_t* face_sel, int32_t* face_src, const int32_t* edges,
                               uint32_t E, const int32_t* edge_offsets, const int32_t* edge_corners, const uint8_t* edge_feature,
                               const uint32_t* vertex_class, const int32_t* ve_offsets, const int32_t* ve_edges, uint64_t* keys, int32_t* quads,
                               uint64_t* vertex_min, uint64_t* total, void* stream) {
    N2M_NOTNULL(total);
    hipStream_t s = (hipStream_t)stream;
    N2M_HIP(hipMemsetAsync(total, 0, sizeof(uint64_t), s));
    if (E == 0 || V == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(faces); N2M_NOTNULL(face_sel); N2M_NOTNULL(face_src); N2M_NOTNULL(edges); N2M_NOTNULL(edge_offsets);
    N2M_NOTNULL(edge_corners); N2M_NOTNULL(edge_feature); N2M_NOTNULL(vertex_class); N2M_NOTNULL(ve_offsets); N2M_NOTNULL(ve_edges);
    N2M_NOTNULL(keys); N2M_NOTNULL(quads); N2M_NOTNULL(vertex_min);
    N2M_HIP(hipMemsetAsync(vertex_min, 0xff, (size_t)V * sizeof(uint64_t), s));
    rm_flip_candidates_kernel<<<grid_of(E), kRmBlock, 0, s>>>(vertices, faces, face_sel, edges, E, edge_offsets, edge_corners, edge_feature,
                                                             vertex_class, ve_offsets, ve_edges, keys, quads, (unsigned long long*)vertex_min);
    N2M_CHECK_LAUNCH();
    rm_flip_apply_kernel<<<grid_of(E), kRmBlock, 0, s>>>(E, keys, quads, (const unsigned long long*)vertex_min, faces, face_src,
                                                        (unsigned long long*)total);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_remesh_relax(const float* vertices, uint32_t V, const int32_t* faces, const int32_t* edges, const uint32_t* vertex_class,
                          const int32_t* vf_offsets, const int32_t* vf_faces, const int32_t* ve_offsets, const int32_t* ve_edges, float* out,
                          uint8_t* moved, double* vertex_normals, void* stream) {
    if (V == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(vertex_class); N2M_NOTNULL(vf_offsets); N2M_NOTNULL(ve_offsets); N2M_NOTNULL(out); N2M_NOTNULL(moved);
    N2M_NOTNULL(vertex_normals);
    N2M_REQUIRE(out != vertices, N2M_EINVAL, "%s: out must not alias vertices (a Jacobi step reads the old positions)", __func__);
    rm_relax_kernel<<<grid_of(V), kRmBlock, 0, (hipStream_t)stream>>>(vertices, faces, edges, vertex_class, vf_offsets, vf_faces, ve_offsets,
                                                                    ve_edges, V, out, moved, vertex_normals);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_remesh_relax_revert(const float* before, float* vertices, uint32_t V, const int32_t* faces, uint32_t F, uint8_t* moved,
                                 const double* vertex_normals, uint8_t* revert, uint64_t* total, void* stream) {
    N2M_NOTNULL(total);
    hipStream_t s = (hipStream_t)stream;
    N2M_HIP(hipMemsetAsync(total, 0, sizeof(uint64_t), s));
    if (V == 0 || F == 0) return 0;
    N2M_NOTNULL(before); N2M_NOTNULL(vertices); N2M_NOTNULL(faces); N2M_NOTNULL(moved); N2M_NOTNULL(vertex_normals); N2M_NOTNULL(revert);
    N2M_HIP(hipMemsetAsync(revert, 0, V, s));
    rm_relax_offending_kernel<<<grid_of(F), kRmBlock, 0, s>>>(before, vertices, faces, F, moved, vertex_normals, revert);
    N2M_CHECK_LAUNCH();
    rm_relax_revert_kernel<<<grid_of(V), kRmBlock, 0, s>>>(before, vertices, V, moved, revert, (unsigned long long*)total);
    N2M_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
