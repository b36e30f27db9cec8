// Mesh decimation and midpoint subdivision on the device: what the reference does on the host with pymeshlab
// (`meshing_decimation_quadric_edge_collapse`, `meshing_surface_subdivision_midpoint`; meshutils.py:191-231, nerf/renderer.py:209-294,
// :540-541, :582-583, :658-659).  The passes below are the per-element work; sorting edge keys, unique-ing them and the CSR offsets are
// torch plumbing in nerf2mesh_amd/mesh_simplify.py, which also drives the rounds.  DESIGN.md section 4.11 states the rule; the numpy
// restatement in tests/mesh_simplify_ref.py reproduces it bit for bit.
//
// Mesh: vertices f32 [V][3], faces i32 [F][3].  Corner k of a face owns the edge (v_k, v_{k+1 mod 3}); c2e [F][3] is that edge's id.
// Edges [E][2] i32 with a < b, in ascending (a, b) order; nf [E] = number of faces on the edge.  CSR: vertex -> incident faces (ascending
// face id), vertex -> incident edges (ascending neighbour id).
//
// Every value a selection depends on is computed in fp64 with + - * / and one sqrt per face quadric, all IEEE correctly rounded on
// gfx950 (division: v_div_scale / v_rcp / fma / v_div_fmas / v_div_fixup; sqrt: the backend's refined expansion), no FMA contraction
// (-ffp-contract=off), no float atomics.  The only atomics are integer ORs and adds whose results do not depend on their order.
#include <math.h>

#include "n2m_common.hpp"

namespace {

constexpr uint32_t kMsBlock = 256;
constexpr uint32_t kFrozen = 1u, kBoundary = 2u;
constexpr uint64_t kNoKey = ~0ull;

struct D3 { double x, y, z; };

__device__ __forceinline__ D3 ld3(const float* __restrict__ v, int32_t i) {
    return D3{(double)v[3 * (int64_t)i], (double)v[3 * (int64_t)i + 1], (double)v[3 * (int64_t)i + 2]};
}
__device__ __forceinline__ D3 sub(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// Q += s * p p^T for the plane p = (n, d): coefficients a2 ab ac ad b2 bc bd c2 cd d2 (terms rounded as (n_i * n_j) * s)
__device__ __forceinline__ void add_plane(double q[10], D3 n, double d, double s) {
    q[0] += (n.x * n.x) * s; q[1] += (n.x * n.y) * s; q[2] += (n.x * n.z) * s; q[3] += (n.x * d) * s;
    q[4] += (n.y * n.y) * s; q[5] += (n.y * n.z) * s; q[6] += (n.y * d) * s;
    q[7] += (n.z * n.z) * s; q[8] += (n.z * d) * s; q[9] += (d * d) * s;
}

// v^T Q v with v = (x, y, z, 1), evaluated row by row in this order
__device__ __forceinline__ double quadric_cost(const double q[10], D3 p) {
    const double r0 = q[0] * p.x + q[1] * p.y + q[2] * p.z + q[3];
    const double r1 = q[1] * p.x + q[4] * p.y + q[5] * p.z + q[6];
    const double r2 = q[2] * p.x + q[5] * p.y + q[7] * p.z + q[8];
    const double r3 = q[3] * p.x + q[6] * p.y + q[8] * p.z + q[9];
    return p.x * r0 + p.y * r1 + p.z * r2 + r3;
}

// Tie-break of the selection key: a bijection of the 32-bit edge id (murmur3's finaliser: xor-shifts and odd multiplies).  Keys stay
// unique; edges of equal cost (exactly zero on every flat region) are ordered pseudo-randomly instead of by id -- ordered ids make the
// local minima of a flat region's 2-rings rare (one per run of ascending ids), and the rounds there stall at a few dozen collapses.
__device__ __forceinline__ uint32_t mix_id(uint32_t h) {
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

__device__ __forceinline__ D3 round_f32(D3 p) { return D3{(double)(float)p.x, (double)(float)p.y, (double)(float)p.z}; }

// ------------------------------------------------------------------------------------------------------------ vertex flags
__global__ void ms_vertex_flags_kernel(const int32_t* __restrict__ faces, uint32_t F, const int32_t* __restrict__ c2e,
                                       const int32_t* __restrict__ nf, const uint8_t* __restrict__ face_sel, uint32_t* __restrict__ flags) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const bool outside = face_sel != nullptr && face_sel[f] == 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t v0 = faces[3 * (int64_t)f + k], v1 = faces[3 * (int64_t)f + (k + 1) % 3];
        const int32_t n = nf[c2e[3 * (int64_t)f + k]];
        const uint32_t m = (n > 2 ? kFrozen : 0u) | (n == 1 ? kBoundary : 0u);
        if (m) { atomicOr(flags + v0, m); atomicOr(flags + v1, m); }
        if (outside) atomicOr(flags + v0, kFrozen);
    }
}

// ------------------------------------------------------------------------------------------------------------ quadrics
// One thread per vertex, faces in ascending id: the face's area-weighted plane quadric, then (corner order: the edge leaving v, the edge
// entering v) Garland's perpendicular constraint plane of every boundary edge at v.
__global__ void ms_quadrics_kernel(const float* __restrict__ verts, uint32_t V, const int32_t* __restrict__ faces,
                                   const int32_t* __restrict__ c2e, const int32_t* __restrict__ nf, const int32_t* __restrict__ vf_off,
                                   const int32_t* __restrict__ vf_idx, double boundary_weight, double* __restrict__ Q) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    double q[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int32_t j = vf_off[v]; j < vf_off[v + 1]; ++j) {
        const int32_t f = vf_idx[j];
        const int32_t* t = faces + 3 * (int64_t)f;
        const D3 p0 = ld3(verts, t[0]), p1 = ld3(verts, t[1]), p2 = ld3(verts, t[2]);
        const D3 n = cross(sub(p1, p0), sub(p2, p0));
        const double nn = dot(n, n);
        if (nn > 0.0) {
            const double d = -dot(n, p0);
            add_plane(q, n, d, 0.5 / sqrt(nn));                // area/|n|^2 = 0.5/|n|: the plane of unit normal, weighted by the area
        }
        const int k = t[0] == (int32_t)v ? 0 : (t[1] == (int32_t)v ? 1 : 2);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = h == 0 ? k : (k + 2) % 3;            // corner owning the edge: leaving v, then entering v
            if (nf[c2e[3 * (int64_t)f + c]] != 1) continue;
            const D3 a = ld3(verts, t[c]), b = ld3(verts, t[(c + 1) % 3]);
            const D3 e = sub(b, a);
            const D3 m = cross(e, n);                          // in the edge, perpendicular to the face
            const double mm = dot(m, m);
            if (!(mm > 0.0)) continue;
            add_plane(q, m, -dot(m, a), (boundary_weight * dot(e, e)) / mm);   // unit plane weighted by |e|^2 * boundary_weight
        }
    }
    for (int i = 0; i < 10; ++i) Q[10 * (int64_t)v + i] = q[i];
}

// ------------------------------------------------------------------------------------------------------------ edge cost
__device__ __forceinline__ bool star_flips(const float* __restrict__ verts, const int32_t* __restrict__ faces, const int32_t* __restrict__ vf_off,
                                           const int32_t* __restrict__ vf_idx, int32_t v, int32_t a, int32_t b, D3 p) {
    for (int32_t j = vf_off[v]; j < vf_off[v + 1]; ++j) {
        const int32_t* t = faces + 3 * (int64_t)vf_idx[j];
        const bool has_a = t[0] == a || t[1] == a || t[2] == a, has_b = t[0] == b || t[1] == b || t[2] == b;
        if (has_a && has_b) continue;                          // dies with the collapse
        D3 o[3], w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = ld3(verts, t[k]);
            w[k] = (t[k] == a || t[k] == b) ? p : o[k];
        }
        const D3 n0 = cross(sub(o[1], o[0]), sub(o[2], o[0]));
        const D3 n1 = cross(sub(w[1], w[0]), sub(w[2], w[0]));
        if (!(dot(n1, n0) > 0.0)) return true;
    }
    return false;
}

__global__ void ms_edge_cost_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, const int32_t* __restrict__ edges,
                                    const int32_t* __restrict__ nf, uint32_t E, const uint32_t* __restrict__ flags, const double* __restrict__ Q,
                                    const int32_t* __restrict__ vf_off, const int32_t* __restrict__ vf_idx, const int32_t* __restrict__ ve_off,
                                    const int32_t* __restrict__ ve_idx, int optimal, uint64_t* __restrict__ keys, float* __restrict__ placement) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int32_t a = edges[2 * (int64_t)e], b = edges[2 * (int64_t)e + 1];
    const int32_t n = nf[e];
    keys[e] = kNoKey;
    const uint32_t fa = flags[a], fb = flags[b];
    if (n > 2 || ((fa | fb) & kFrozen)) return;
    if (n == 2 && (fa & kBoundary) && (fb & kBoundary)) return;   // link condition with the virtual vertex behind the boundary
    // link condition: common neighbours of a and b == faces on the edge (both lists ascending by neighbour id)
    int32_t common = 0;
    {
        int32_t i = ve_off[a], j = ve_off[b];
        const int32_t ie = ve_off[a + 1], je = ve_off[b + 1];
        while (i < ie && j < je) {
            const int32_t ea = ve_idx[i], eb = ve_idx[j];
            const int32_t na = edges[2 * (int64_t)ea] ^ edges[2 * (int64_t)ea + 1] ^ a;
            const int32_t nb = edges[2 * (int64_t)eb] ^ edges[2 * (int64_t)eb + 1] ^ b;
            if (na == nb) { ++common; ++i; ++j; }
            else if (na < nb) ++i;
            else ++j;
        }
    }
    if (common != n) return;

    double q[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) q[i] = Q[10 * (int64_t)a + i] + Q[10 * (int64_t)b + i];
    const D3 pa = ld3(verts, a), pb = ld3(verts, b);
    const D3 mid = D3{(pa.x + pb.x) * 0.5, (pa.y + pb.y) * 0.5, (pa.z + pb.z) * 0.5};
    D3 p;
    bool solved = false;
    if (optimal) {
        const double c00 = q[4] * q[7] - q[5] * q[5], c01 = q[5] * q[2] - q[1] * q[7], c02 = q[1] * q[5] - q[4] * q[2];
        const double c11 = q[0] * q[7] - q[2] * q[2], c12 = q[2] * q[1] - q[0] * q[5], c22 = q[0] * q[4] - q[1] * q[1];
        const double det = q[0] * c00 + q[1] * c01 + q[2] * c02;
        const double tr = q[0] + q[4] + q[7];
        if (fabs(det) > 1e-12 * (tr * tr * tr)) {
            const double r0 = -q[3], r1 = -q[6], r2 = -q[8];
            const D3 x = D3{(c00 * r0 + c01 * r1 + c02 * r2) / det, (c01 * r0 + c11 * r1 + c12 * r2) / det,
                            (c02 * r0 + c12 * r1 + c22 * r2) / det};
            const D3 dm = sub(x, mid), ab = sub(pb, pa);
            if (dot(dm, dm) <= 4.0 * dot(ab, ab)) {             // within two edge lengths of the midpoint
                p = round_f32(x);
                solved = true;
            }
        }
    }
    double cost;
    if (solved) {
        cost = quadric_cost(q, p);
    } else {
        const D3 pm = round_f32(mid);
        const double ca = quadric_cost(q, pa), cb = quadric_cost(q, pb), cm = quadric_cost(q, pm);
        p = pa; cost = ca;
        if (cb < cost) { p = pb; cost = cb; }
        if (cm < cost) { p = pm; cost = cm; }
    }
    if (star_flips(verts, faces, vf_off, vf_idx, a, a, b, p) || star_flips(verts, faces, vf_off, vf_idx, b, a, b, p)) return;
    const float c32 = (float)(cost > 0.0 ? cost : 0.0);
    keys[e] = ((uint64_t)__float_as_uint(c32) << 32) | (uint64_t)mix_id(e);
    placement[3 * (int64_t)e] = (float)p.x;
    placement[3 * (int64_t)e + 1] = (float)p.y;
    placement[3 * (int64_t)e + 2] = (float)p.z;
}

// ------------------------------------------------------------------------------------------------------------ independent set
// pass 1 (closed = 0): m[v] = min key over the edges at v.  pass 2 (closed = 1): m[v] = min of src over v and its neighbours.
__global__ void ms_vertex_min_kernel(const int32_t* __restrict__ edges, const int32_t* __restrict__ ve_off, const int32_t* __restrict__ ve_idx,
                                     uint32_t V, const uint64_t* __restrict__ src, int closed, uint64_t* __restrict__ dst) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    uint64_t m = closed ? src[v] : kNoKey;
    for (int32_t j = ve_off[v]; j < ve_off[v + 1]; ++j) {
        const int32_t e = ve_idx[j];
        const uint64_t k = closed ? src[edges[2 * (int64_t)e] ^ edges[2 * (int64_t)e + 1] ^ (int32_t)v] : src[e];
        m = k < m ? k : m;
    }
    dst[v] = m;
}

__global__ void ms_select_kernel(const int32_t* __restrict__ edges, const int32_t* __restrict__ nf, uint32_t E, const uint64_t* __restrict__ keys,
                                 const uint64_t* __restrict__ m2, uint8_t* __restrict__ sel, unsigned long long* __restrict__ totals) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const uint64_t k = keys[e];
    const bool s = k != kNoKey && k == m2[edges[2 * (int64_t)e]] && k == m2[edges[2 * (int64_t)e + 1]];
    sel[e] = s ? 1 : 0;
    if (s) {
        atomicAdd(totals, 1ull);
        atomicAdd(totals + 1, (unsigned long long)nf[e]);
    }
}

// ------------------------------------------------------------------------------------------------------------ collapse
__global__ void ms_collapse_kernel(const int32_t* __restrict__ edges, uint32_t E, const uint8_t* __restrict__ sel,
                                   const float* __restrict__ placement, float* __restrict__ verts, double* __restrict__ Q,
                                   int32_t* __restrict__ dest) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E || !sel[e]) return;
    const int32_t a = edges[2 * (int64_t)e], b = edges[2 * (int64_t)e + 1];
#pragma unroll
    for (int i = 0; i < 3; ++i) verts[3 * (int64_t)a + i] = placement[3 * (int64_t)e + i];
#pragma unroll
    for (int i = 0; i < 10; ++i) Q[10 * (int64_t)a + i] = Q[10 * (int64_t)a + i] + Q[10 * (int64_t)b + i];
    dest[b] = a;
}

__global__ void ms_repoint_kernel(int32_t* __restrict__ faces, uint32_t F, const int32_t* __restrict__ dest, uint8_t* __restrict__ alive) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    int32_t t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t v = faces[3 * (int64_t)f + k];
        const int32_t d = dest[v];
        t[k] = d >= 0 ? d : v;
        faces[3 * (int64_t)f + k] = t[k];
    }
    alive[f] = (t[0] != t[1] && t[1] != t[2] && t[2] != t[0]) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ compaction
// Row i of `src` [n][width] with keep[i] goes to row scan[i] (the inclusive prefix sum of keep, minus one) of dst: stable.
template <typename T>
__global__ void ms_compact_rows_kernel(const T* __restrict__ src, uint32_t n, uint32_t width, const uint8_t* __restrict__ keep,
                                       const int32_t* __restrict__ scan, T* __restrict__ dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const int64_t o = (int64_t)(scan[i] - 1);
    for (uint32_t c = 0; c < width; ++c) dst[o * width + c] = src[(int64_t)i * width + c];
}

__global__ void ms_mark_referenced_kernel(const int32_t* __restrict__ faces, uint32_t F, uint8_t* __restrict__ ref) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3u * F) return;
    ref[faces[i]] = 1;
}

__global__ void ms_reindex_kernel(int32_t* __restrict__ faces, uint32_t n, const int32_t* __restrict__ scan) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    faces[i] = scan[faces[i]] - 1;
}

// ------------------------------------------------------------------------------------------------------------ subdivision
__global__ void ms_subdiv_mark_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, uint32_t F,
                                      const int32_t* __restrict__ c2e, const uint8_t* __restrict__ face_sel, double thr2,
                                      uint8_t* __restrict__ split) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F || !face_sel[f]) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const D3 d = sub(ld3(verts, faces[3 * (int64_t)f + (k + 1) % 3]), ld3(verts, faces[3 * (int64_t)f + k]));
        if (dot(d, d) > thr2) split[c2e[3 * (int64_t)f + k]] = 1;
    }
}

__global__ void ms_subdiv_midpoints_kernel(float* __restrict__ verts, uint32_t V, const int32_t* __restrict__ edges, uint32_t E,
                                           const uint8_t* __restrict__ split, const int32_t* __restrict__ split_scan) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E || !split[e]) return;
    const D3 a = ld3(verts, edges[2 * (int64_t)e]), b = ld3(verts, edges[2 * (int64_t)e + 1]);
    const int64_t o = 3 * ((int64_t)V + split_scan[e] - 1);
    verts[o] = (float)((a.x + b.x) * 0.5);
    verts[o + 1] = (float)((a.y + b.y) * 0.5);
    verts[o + 2] = (float)((a.z + b.z) * 0.5);
}

__device__ __forceinline__ uint32_t split_pattern(const int32_t* __restrict__ c2e, const uint8_t* __restrict__ split, uint32_t f) {
    return (split[c2e[3 * (int64_t)f]] ? 1u : 0u) | (split[c2e[3 * (int64_t)f + 1]] ? 2u : 0u) | (split[c2e[3 * (int64_t)f + 2]] ? 4u : 0u);
}

__global__ void ms_subdiv_count_kernel(const int32_t* __restrict__ c2e, uint32_t F, const uint8_t* __restrict__ split,
                                       int32_t* __restrict__ counts) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    counts[f] = 1 + __popc(split_pattern(c2e, split, f));
}

// Children of face (v0, v1, v2), m_k = midpoint of the edge (v_k, v_k+1):
//   none split  (v0, v1, v2)
//   edge k      (v_k, m_k, v_k+2), (m_k, v_k+1, v_k+2)
//   all three   (v0, m0, m2), (v1, m1, m0), (v2, m2, m1), (m0, m1, m2)
//   all but k   corner (m_k+1, v_k+2, m_k+2); the quad v_k v_k+1 m_k+1 m_k+2 is cut by its shorter diagonal, (v_k, m_k+1) on a tie:
//               (v_k, v_k+1, m_k+1), (v_k, m_k+1, m_k+2)   or   (v_k, v_k+1, m_k+2), (v_k+1, m_k+1, m_k+2)
__global__ void ms_subdiv_emit_kernel(const float* __restrict__ verts, uint32_t V, const int32_t* __restrict__ faces, uint32_t F,
                                      const int32_t* __restrict__ c2e, const uint8_t* __restrict__ split, const int32_t* __restrict__ split_scan,
                                      const int32_t* __restrict__ face_scan, const uint8_t* __restrict__ face_sel, int32_t* __restrict__ out,
                                      uint8_t* __restrict__ out_sel) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const uint32_t pat = split_pattern(c2e, split, f);
    const int32_t* t = faces + 3 * (int64_t)f;
    int32_t m[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] = ((pat >> k) & 1u) ? (int32_t)V + split_scan[c2e[3 * (int64_t)f + k]] - 1 : -1;
    const int nc = 1 + __popc(pat);
    int32_t c[4][3];
    if (pat == 0u) {
        c[0][0] = t[0]; c[0][1] = t[1]; c[0][2] = t[2];
    } else if (pat == 7u) {
        c[0][0] = t[0]; c[0][1] = m[0]; c[0][2] = m[2];
        c[1][0] = t[1]; c[1][1] = m[1]; c[1][2] = m[0];
        c[2][0] = t[2]; c[2][1] = m[2]; c[2][2] = m[1];
        c[3][0] = m[0]; c[3][1] = m[1]; c[3][2] = m[2];
    } else if (__popc(pat) == 1) {
        const int k = pat == 1u ? 0 : (pat == 2u ? 1 : 2);
        const int32_t vk = t[k], vk1 = t[(k + 1) % 3], vk2 = t[(k + 2) % 3];
        c[0][0] = vk; c[0][1] = m[k]; c[0][2] = vk2;
        c[1][0] = m[k]; c[1][1] = vk1; c[1][2] = vk2;
    } else {
        const int k = pat == 6u ? 0 : (pat == 5u ? 1 : 2);    // the unsplit edge
        const int32_t vk = t[k], vk1 = t[(k + 1) % 3], vk2 = t[(k + 2) % 3];
        const int32_t m1 = m[(k + 1) % 3], m2 = m[(k + 2) % 3];
        c[0][0] = m1; c[0][1] = vk2; c[0][2] = m2;
        const D3 d1 = sub(ld3(verts, m1), ld3(verts, vk)), d2 = sub(ld3(verts, m2), ld3(verts, vk1));
        if (dot(d1, d1) <= dot(d2, d2)) {
            c[1][0] = vk; c[1][1] = vk1; c[1][2] = m1;
            c[2][0] = vk; c[2][1] = m1; c[2][2] = m2;
        } else {
            c[1][0] = vk; c[1][1] = vk1; c[1][2] = m2;
            c[2][0] = vk1; c[2][1] = m1; c[2][2] = m2;
        }
    }
    const int64_t o = face_scan[f] - nc;                        // inclusive scan of the child counts
    const uint8_t s = face_sel ? face_sel[f] : 0;
    for (int i = 0; i < nc; ++i) {
        out[3 * (o + i)] = c[i][0]; out[3 * (o + i) + 1] = c[i][1]; out[3 * (o + i) + 2] = c[i][2];
        if (out_sel) out_sel[o + i] = s;
    }
}

inline uint32_t grid_of(uint64_t n) { return n2m_ceil_div(n, kMsBlock); }

}  // namespace

extern "C" {

int n2m_mesh_vertex_flags(const int32_t* faces, uint32_t F, const int32_t* c2e, const int32_t* edge_nf, const uint8_t* face_sel, uint32_t V,
                          uint32_t* flags, void* stream) {
    N2M_NOTNULL(flags);
    if (F) { N2M_NOTNULL(faces); N2M_NOTNULL(c2e); N2M_NOTNULL(edge_nf); }
    hipStream_t s = (hipStream_t)stream;
    if (V) N2M_HIP(hipMemsetAsync(flags, 0, (size_t)V * sizeof(uint32_t), s));
    if (F == 0) return 0;
    ms_vertex_flags_kernel<<<grid_of(F), kMsBlock, 0, s>>>(faces, F, c2e, edge_nf, face_sel, flags);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_quadrics(const float* vertices, uint32_t V, const int32_t* faces, const int32_t* c2e, const int32_t* edge_nf,
                      const int32_t* vf_offsets, const int32_t* vf_faces, double boundary_weight, double* quadrics, void* stream) {
    if (V == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(faces); N2M_NOTNULL(c2e); N2M_NOTNULL(edge_nf); N2M_NOTNULL(vf_offsets); N2M_NOTNULL(vf_faces);
    N2M_NOTNULL(quadrics);
    N2M_REQUIRE(boundary_weight >= 0.0, N2M_EINVAL, "%s: boundary_weight must be >= 0", __func__);
    hipStream_t s = (hipStream_t)stream;
    ms_quadrics_kernel<<<grid_of(V), kMsBlock, 0, s>>>(vertices, V, faces, c2e, edge_nf, vf_offsets, vf_faces, boundary_weight, quadrics);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_edge_collapse_cost(const float* vertices, const int32_t* faces, const int32_t* edges, const int32_t* edge_nf, uint32_t E,
                                const uint32_t* flags, const double* quadrics, const int32_t* vf_offsets, const int32_t* vf_faces,
                                const int32_t* ve_offsets, const int32_t* ve_edges, int optimal_placement, uint64_t* keys, float* placement,
                                void* stream) {
    if (E == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(faces); N2M_NOTNULL(edges); N2M_NOTNULL(edge_nf); N2M_NOTNULL(flags); N2M_NOTNULL(quadrics);
    N2M_NOTNULL(vf_offsets); N2M_NOTNULL(vf_faces); N2M_NOTNULL(ve_offsets); N2M_NOTNULL(ve_edges); N2M_NOTNULL(keys); N2M_NOTNULL(placement);
    hipStream_t s = (hipStream_t)stream;
    ms_edge_cost_kernel<<<grid_of(E), kMsBlock, 0, s>>>(vertices, faces, edges, edge_nf, E, flags, quadrics, vf_offsets, vf_faces, ve_offsets,
                                                        ve_edges, optimal_placement, keys, placement);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_select_collapses(const int32_t* edges, const int32_t* edge_nf, uint32_t E, const uint64_t* keys, const int32_t* ve_offsets,
                              const int32_t* ve_edges, uint32_t V, void* workspace, uint64_t workspace_bytes, uint8_t* selected,
                              uint64_t* totals, void* stream) {
    N2M_NOTNULL(totals);
    N2M_REQUIRE(workspace_bytes >= 2ull * V * sizeof(uint64_t), N2M_EINVAL, "%s: workspace needs 16 bytes per vertex", __func__);
    hipStream_t s = (hipStream_t)stream;
    N2M_HIP(hipMemsetAsync(totals, 0, 2 * sizeof(uint64_t), s));
    if (E == 0 || V == 0) return 0;
    N2M_NOTNULL(edges); N2M_NOTNULL(edge_nf); N2M_NOTNULL(keys); N2M_NOTNULL(ve_offsets); N2M_NOTNULL(ve_edges); N2M_NOTNULL(workspace);
    N2M_NOTNULL(selected);
    uint64_t* m1 = (uint64_t*)workspace;
    uint64_t* m2 = m1 + V;
    ms_vertex_min_kernel<<<grid_of(V), kMsBlock, 0, s>>>(edges, ve_offsets, ve_edges, V, keys, 0, m1);
    N2M_CHECK_LAUNCH();
    ms_vertex_min_kernel<<<grid_of(V), kMsBlock, 0, s>>>(edges, ve_offsets, ve_edges, V, m1, 1, m2);
    N2M_CHECK_LAUNCH();
    ms_select_kernel<<<grid_of(E), kMsBlock, 0, s>>>(edges, edge_nf, E, keys, m2, selected, (unsigned long long*)totals);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_collapse_apply(const int32_t* edges, uint32_t E, const uint8_t* selected, const float* placement, float* vertices, double* quadrics,
                            uint32_t V, int32_t* faces, uint32_t F, int32_t* dest, uint8_t* face_alive, void* stream) {
    if (F == 0) return 0;
    N2M_NOTNULL(edges); N2M_NOTNULL(selected); N2M_NOTNULL(placement); N2M_NOTNULL(vertices); N2M_NOTNULL(quadrics); N2M_NOTNULL(faces);
    N2M_NOTNULL(dest); N2M_NOTNULL(face_alive);
    hipStream_t s = (hipStream_t)stream;
    N2M_HIP(hipMemsetAsync(dest, 0xff, (size_t)V * sizeof(int32_t), s));
    if (E) {
        ms_collapse_kernel<<<grid_of(E), kMsBlock, 0, s>>>(edges, E, selected, placement, vertices, quadrics, dest);
        N2M_CHECK_LAUNCH();
    }
    ms_repoint_kernel<<<grid_of(F), kMsBlock, 0, s>>>(faces, F, dest, face_alive);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_compact_rows(const void* src, uint32_t n, uint32_t width, uint32_t elem_bytes, const uint8_t* keep, const int32_t* scan, void* dst,
                          void* stream) {
    if (n == 0 || width == 0) return 0;
    N2M_NOTNULL(src); N2M_NOTNULL(keep); N2M_NOTNULL(scan); N2M_NOTNULL(dst);
    hipStream_t s = (hipStream_t)stream;
    if (elem_bytes == 4) ms_compact_rows_kernel<uint32_t><<<grid_of(n), kMsBlock, 0, s>>>((const uint32_t*)src, n, width, keep, scan, (uint32_t*)dst);
    else if (elem_bytes == 8) ms_compact_rows_kernel<uint64_t><<<grid_of(n), kMsBlock, 0, s>>>((const uint64_t*)src, n, width, keep, scan, (uint64_t*)dst);
    else if (elem_bytes == 1) ms_compact_rows_kernel<uint8_t><<<grid_of(n), kMsBlock, 0, s>>>((const uint8_t*)src, n, width, keep, scan, (uint8_t*)dst);
    else N2M_REQUIRE(false, N2M_EINVAL, "%s: elem_bytes must be 1, 4 or 8", __func__);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_mark_referenced(const int32_t* faces, uint32_t F, uint32_t V, uint8_t* referenced, void* stream) {
    N2M_NOTNULL(referenced);
    hipStream_t s = (hipStream_t)stream;
    if (V) N2M_HIP(hipMemsetAsync(referenced, 0, V, s));
    if (F == 0) return 0;
    N2M_NOTNULL(faces);
    ms_mark_referenced_kernel<<<grid_of(3ull * F), kMsBlock, 0, s>>>(faces, F, referenced);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_reindex(int32_t* indices, uint32_t n, const int32_t* scan, void* stream) {
    if (n == 0) return 0;
    N2M_NOTNULL(indices); N2M_NOTNULL(scan);
    ms_reindex_kernel<<<grid_of(n), kMsBlock, 0, (hipStream_t)stream>>>(indices, n, scan);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_subdiv_mark(const float* vertices, const int32_t* faces, uint32_t F, const int32_t* c2e, const uint8_t* face_sel, double threshold_sq,
                         uint32_t E, uint8_t* split, void* stream) {
    N2M_NOTNULL(split);
    hipStream_t s = (hipStream_t)stream;
    if (E) N2M_HIP(hipMemsetAsync(split, 0, E, s));
    if (F == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(faces); N2M_NOTNULL(c2e); N2M_NOTNULL(face_sel);
    ms_subdiv_mark_kernel<<<grid_of(F), kMsBlock, 0, s>>>(vertices, faces, F, c2e, face_sel, threshold_sq, split);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_subdiv_midpoints(float* vertices, uint32_t V, const int32_t* edges, uint32_t E, const uint8_t* split, const int32_t* split_scan,
                              void* stream) {
    if (E == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(edges); N2M_NOTNULL(split); N2M_NOTNULL(split_scan);
    ms_subdiv_midpoints_kernel<<<grid_of(E), kMsBlock, 0, (hipStream_t)stream>>>(vertices, V, edges, E, split, split_scan);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_subdiv_count(const int32_t* c2e, uint32_t F, const uint8_t* split, int32_t* counts, void* stream) {
    if (F == 0) return 0;
    N2M_NOTNULL(c2e); N2M_NOTNULL(split); N2M_NOTNULL(counts);
    ms_subdiv_count_kernel<<<grid_of(F), kMsBlock, 0, (hipStream_t)stream>>>(c2e, F, split, counts);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_subdiv_emit(const float* vertices, uint32_t V, const int32_t* faces, uint32_t F, const int32_t* c2e, const uint8_t* split,
                         const int32_t* split_scan, const int32_t* face_scan, const uint8_t* face_sel, int32_t* out_faces, uint8_t* out_sel,
                         void* stream) {
    if (F == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(faces); N2M_NOTNULL(c2e); N2M_NOTNULL(split); N2M_NOTNULL(split_scan); N2M_NOTNULL(face_scan);
    N2M_NOTNULL(out_faces);
    ms_subdiv_emit_kernel<<<grid_of(F), kMsBlock, 0, (hipStream_t)stream>>>(vertices, V, faces, F, c2e, split, split_scan, face_scan, face_sel,
                                                                          out_faces, out_sel);
    N2M_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
