// Mesh cleaning on the device: what the reference does on the host with pymeshlab in `clean_mesh` (meshutils.py:146-188; called by
// nerf/renderer.py:537, :653): merge close vertices, remove duplicate and null faces, remove small connected components, repair
// non-manifold edges and vertices.  The passes below are the per-element work; sorting keys, unique-ing edges and the CSR offsets are
// torch plumbing in nerf2mesh_amd/mesh_clean.py, which also drives the rounds.  DESIGN.md section 4.12 states the rule; the sequential
// numpy restatement in tests/mesh_clean_ref.py reproduces it bit for bit.
//
// Mesh: vertices f32 [V][3], faces i32 [F][3]; c2e [F][3] = edge id of the corner's edge (v_k, v_k+1), nf [E] = faces on the edge.
// Every comparison that decides something is an exact fp64 evaluation of fp32 inputs (or one correctly rounded sqrt) or an integer
// compare; no float atomics.  The integer atomics (min, max, add, compare-and-swap of union-find roots) give results that do not depend
// on their order.  Every round reads the previous round's state and writes a second buffer, so round counts do not depend on thread
// timing either.
#include <math.h>

#include "n2m_mesh.hpp"

namespace {

constexpr uint32_t kMcBlock = 256;
constexpr int32_t kUndecided = -1;
constexpr int32_t kNone = 0x7fffffff;

inline uint32_t grid_of(uint64_t n) { return n2m_ceil_div(n, kMcBlock); }

// ------------------------------------------------------------------------------------------------------------ merge close vertices
// Cell of a vertex: floor((p - lo) / h) per axis in fp64, clamped to the grid.  h > r, so two points closer than r land in cells at most
// one apart whatever the rounding of the division; clamping is monotone and keeps that.
__device__ __forceinline__ int32_t cell_coord(double p, double lo, double h, int32_t n) {
    const double c = floor((p - lo) / h);
    return c < 0.0 ? 0 : (c >= (double)n ? n - 1 : (int32_t)c);
}

__global__ void mc_cell_keys_kernel(const float* __restrict__ verts, uint32_t V, double lox, double loy, double loz, double h, int32_t nx,
                                    int32_t ny, int32_t nz, int64_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    const int64_t cx = cell_coord(ldc(verts, i, 0), lox, h, nx), cy = cell_coord(ldc(verts, i, 1), loy, h, ny),
                  cz = cell_coord(ldc(verts, i, 2), loz, h, nz);
    keys[i] = (cx * ny + cy) * nz + cz;
}

// One round of the lexicographically-first maximal independent set of the r-graph (the greedy sweep's seeds).  state: -1 undecided,
// i seed, s < i mapped to seed s.  Over the neighbours j < i within r: min_seed (state j == j), min_undec (state -1).  min_seed <
// min_undec: mapped to min_seed; neither exists: seed; otherwise wait, remembering min_undec as the blocker.  A waiting vertex whose
// blocker is still undecided skips the scan: every neighbour below the blocker was a decided non-seed at its last scan and still is, so
// the scan would wait again.  Thread t works on the t-th vertex in cell order (neighbouring threads share cells).
__global__ void mc_merge_round_kernel(const float* __restrict__ verts, uint32_t V, const int32_t* __restrict__ order,
                                      const int64_t* __restrict__ keys, const int32_t* __restrict__ cell_off, int32_t nx, int32_t ny,
                                      int32_t nz, double r2, const int32_t* __restrict__ st_in, int32_t* __restrict__ st_out,
                                      int32_t* __restrict__ blocker, uint32_t* __restrict__ undecided) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= V) return;
    const int32_t i = order[t];
    const int32_t s0 = st_in[i];
    if (s0 != kUndecided) { st_out[i] = s0; return; }
    const int32_t b = blocker[i];
    if (b >= 0 && st_in[b] == kUndecided) {
        st_out[i] = kUndecided;
        atomicAdd(undecided, 1u);
        return;
    }
    const double px = ldc(verts, i, 0), py = ldc(verts, i, 1), pz = ldc(verts, i, 2);
    const int64_t key = keys[i];
    const int32_t cz = (int32_t)(key % nz), cy = (int32_t)((key / nz) % ny), cx = (int32_t)(key / ((int64_t)nz * ny));
    int32_t min_seed = kNone, min_undec = kNone;
    for (int32_t x = cx - 1; x <= cx + 1; ++x) {
        if (x < 0 || x >= nx) continue;
        for (int32_t y = cy - 1; y <= cy + 1; ++y) {
            if (y < 0 || y >= ny) continue;
            for (int32_t z = cz - 1; z <= cz + 1; ++z) {
                if (z < 0 || z >= nz) continue;
                const int64_t c = ((int64_t)x * ny + y) * nz + z;
                const int32_t e = cell_off[c + 1];
                for (int32_t q = cell_off[c]; q < e; ++q) {
                    const int32_t j = order[q];
                    if (j >= i || (j >= min_seed && j >= min_undec)) continue;     // cannot lower either minimum
                    const double dx = ldc(verts, j, 0) - px, dy = ldc(verts, j, 1) - py, dz = ldc(verts, j, 2) - pz;
                    if (!((dx * dx + dy * dy) + dz * dz < r2)) continue;
                    const int32_t sj = st_in[j];
                    if (sj == j) min_seed = j < min_seed ? j : min_seed;
                    else if (sj == kUndecided) min_undec = j < min_undec ? j : min_undec;
                }
            }
        }
    }
    int32_t out = kUndecided;
    if (min_seed < min_undec) out = min_seed;
    else if (min_undec == kNone) out = i;
    st_out[i] = out;
    if (out == kUndecided) {
        blocker[i] = min_undec;
        atomicAdd(undecided, 1u);
    }
}

// faces re-pointed to the seeds (state = own id for a seed, the seed's id otherwise); alive <- three distinct corners
__global__ void mc_repoint_kernel(int32_t* __restrict__ faces, uint32_t F, const int32_t* __restrict__ dest, uint8_t* __restrict__ alive) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    int32_t t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t[k] = dest[faces[3 * (int64_t)f + k]];
        faces[3 * (int64_t)f + k] = t[k];
    }
    alive[f] = (t[0] != t[1] && t[1] != t[2] && t[2] != t[0]) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ duplicate / null faces
__device__ __forceinline__ void sorted3(const int32_t* __restrict__ faces, int32_t f, int32_t s[3]) {
    int32_t a = faces[3 * (int64_t)f], b = faces[3 * (int64_t)f + 1], c = faces[3 * (int64_t)f + 2], x;
    if (a > b) { x = a; a = b; b = x; }
    if (b > c) { x = b; b = c; c = x; }
    if (a > b) { x = a; a = b; b = x; }
    s[0] = a; s[1] = b; s[2] = c;
}

// order [F]: face ids sorted by their sorted corner triple, ties in ascending id.  The first face of every group survives; of those, a
// face whose fp64 cross product is exactly zero is null.  alive <- first && !null; totals[0] += duplicates, totals[1] += null faces.
__global__ void mc_dup_null_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, uint32_t F, const int32_t* __restrict__ order,
                                   uint8_t* __restrict__ alive, unsigned long long* __restrict__ totals) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= F) return;
    const int32_t f = order[p];
    bool first = true;
    if (p > 0) {
        int32_t s[3], q[3];
        sorted3(faces, f, s);
        sorted3(faces, order[p - 1], q);
        first = s[0] != q[0] || s[1] != q[1] || s[2] != q[2];
    }
    bool null_face = false;
    if (first) {
        double n[3];
        face_cross(verts, faces, (uint32_t)f, n);
        null_face = n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0;
    }
    alive[f] = (first && !null_face) ? 1 : 0;
    if (!first) atomicAdd(totals, 1ull);
    else if (null_face) atomicAdd(totals + 1, 1ull);
}

// ------------------------------------------------------------------------------------------------------------ connected components
__global__ void mc_edge_min_face_kernel(const int32_t* __restrict__ c2e, uint32_t F, int32_t* __restrict__ rep) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3u * F) return;
    atomicMin(rep + c2e[i], (int32_t)(i / 3));
}

// parent[f] <- f; the box's lower corner <- ~0 (the upper corner was zeroed): the identities of atomic min / max
__global__ void mc_uf_init_kernel(int32_t* __restrict__ parent, uint32_t* __restrict__ box, uint32_t F) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    parent[f] = (int32_t)f;
#pragma unroll
    for (int c = 0; c < 3; ++c) box[6 * (int64_t)f + c] = 0xffffffffu;
}

__global__ void mc_union_kernel(const int32_t* __restrict__ c2e, uint32_t F, const int32_t* __restrict__ rep, int32_t* parent) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3u * F) return;
    const int32_t g = rep[c2e[i]];
    if (g != (int32_t)(i / 3)) uf_unite(parent, (int32_t)(i / 3), g);
}

// label <- root (the component's minimum face id); per root: face count, and the box of the corners in the order-preserving encoding
__global__ void mc_component_stats_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, uint32_t F,
                                          const int32_t* __restrict__ parent, int32_t* __restrict__ label, int32_t* __restrict__ count,
                                          uint32_t* __restrict__ box) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    int32_t x = (int32_t)f, p = parent[x];
    while (p != x) { x = p; p = parent[x]; }
    label[f] = x;
    atomicAdd(count + x, 1);
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t v = faces[3 * (int64_t)f + k];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t e = fenc(verts[3 * (int64_t)v + c]);
            lo[c] = e < lo[c] ? e : lo[c];
            hi[c] = e > hi[c] ? e : hi[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        atomicMin(box + 6 * (int64_t)x + c, lo[c]);
        atomicMax(box + 6 * (int64_t)x + 3 + c, hi[c]);
    }
}

// alive <- the face's component passes both filters: its box diagonal sqrt((dx^2 + dy^2) + dz^2) (fp64) is not below min_diag (when
// use_diag), then its face count is not below min_faces (when min_faces > 0).  totals: components, removed by the diameter (components,
// faces), removed by the face count (components, faces).
__global__ void mc_component_filter_kernel(uint32_t F, const int32_t* __restrict__ label, const int32_t* __restrict__ count,
                                           const uint32_t* __restrict__ box, int use_diag, double min_diag, int32_t min_faces,
                                           uint8_t* __restrict__ alive, unsigned long long* __restrict__ totals) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int32_t r = label[f];
    bool by_diag = false, by_size = false;
    if (use_diag) {
        const uint32_t* b = box + 6 * (int64_t)r;
        const double dx = (double)fdec(b[3]) - (double)fdec(b[0]), dy = (double)fdec(b[4]) - (double)fdec(b[1]),
                     dz = (double)fdec(b[5]) - (double)fdec(b[2]);
        by_diag = sqrt((dx * dx + dy * dy) + dz * dz) < min_diag;
    }
    if (!by_diag && min_faces > 0) by_size = count[r] < min_faces;
    alive[f] = (by_diag || by_size) ? 0 : 1;
    const bool root = r == (int32_t)f;
    if (root) atomicAdd(totals, 1ull);
    if (by_diag) {
        atomicAdd(totals + 2, 1ull);
        if (root) atomicAdd(totals + 1, 1ull);
    }
    if (by_size) {
        atomicAdd(totals + 4, 1ull);
        if (root) atomicAdd(totals + 3, 1ull);
    }
}

// ------------------------------------------------------------------------------------------------------------ non-manifold edges
// da [F] <- the fp64 double area |(b - a) x (c - a)|; state [F] <- 0 (candidate: an edge with > 2 faces) or 1 (kept); totals[0] +=
// candidates
__global__ void mc_nm_edge_init_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, uint32_t F, const int32_t* __restrict__ c2e,
                                       const int32_t* __restrict__ nf, double* __restrict__ da, uint8_t* __restrict__ state,
                                       unsigned long long* __restrict__ totals) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    double n[3];
    face_cross(verts, faces, f, n);
    da[f] = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const bool cand = nf[c2e[3 * (int64_t)f]] > 2 || nf[c2e[3 * (int64_t)f + 1]] > 2 || nf[c2e[3 * (int64_t)f + 2]] > 2;
    state[f] = cand ? 0 : 1;
    if (cand) atomicAdd(totals, 1ull);
}

__device__ __forceinline__ bool key_less(const double* __restrict__ da, int32_t g, int32_t f) {
    return da[g] < da[f] || (da[g] == da[f] && g < f);
}

// One round of the area-ordered deletion: a candidate is decided once every candidate of smaller (double area, id) on its non-manifold
// edges is decided; it is deleted (2) if one of those edges still has > 2 faces: nf minus the smaller faces already deleted.
// ef_off / ef_faces: edge -> faces CSR.  totals[0] += still undecided, totals[1] += deleted this round.
__global__ void mc_nm_edge_round_kernel(uint32_t F, const int32_t* __restrict__ c2e, const int32_t* __restrict__ nf, const int32_t* __restrict__ ef_off,
                                        const int32_t* __restrict__ ef_faces, const double* __restrict__ da, const uint8_t* __restrict__ st_in,
                                        uint8_t* __restrict__ st_out, unsigned long long* __restrict__ totals) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const uint8_t s0 = st_in[f];
    if (s0 != 0) { st_out[f] = s0; return; }
    bool ready = true, del = false;
    for (int k = 0; k < 3 && ready; ++k) {
        const int32_t e = c2e[3 * (int64_t)f + k];
        int32_t live = nf[e];
        if (live <= 2) continue;
        for (int32_t j = ef_off[e]; j < ef_off[e + 1]; ++j) {
            const int32_t g = ef_faces[j];
            if (g == (int32_t)f || !key_less(da, g, (int32_t)f)) continue;
            const uint8_t sg = st_in[g];
            if (sg == 0) { ready = false; break; }
            if (sg == 2) --live;
        }
        if (live > 2) del = true;
    }
    st_out[f] = ready ? (del ? 2 : 1) : 0;
    if (!ready) atomicAdd(totals, 1ull);
    else if (del) atomicAdd(totals + 1, 1ull);
}

// ------------------------------------------------------------------------------------------------------------ non-manifold vertices
// One thread per vertex over its corners vf_corner[vf_off[v] .. vf_off[v+1]) (flat corner ids f * 3 + k, ascending): walk the fan of
// the first corner through the edges (v, w) it shares with the other incident faces.  visited [3F] (aligned with vf_corner) <- the
// corner is in that fan; stack [3F] is the walk's scratch, inside the vertex's own range.  split[v] <- some incident corner is outside
// the fan; first[v] <- the first corner (INT32_MAX for an unreferenced vertex).
__global__ void mc_fan_walk_kernel(const int32_t* __restrict__ faces, uint32_t V, const int32_t* __restrict__ vf_off, const int32_t* __restrict__ vf_corner,
                                   uint8_t* __restrict__ visited, int32_t* __restrict__ stack, uint8_t* __restrict__ split, int32_t* __restrict__ first,
                                   unsigned long long* __restrict__ totals) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int32_t o = vf_off[v], e = vf_off[v + 1];
    split[v] = 0;
    first[v] = o < e ? vf_corner[o] : kNone;
    if (o >= e) return;
    for (int32_t j = o; j < e; ++j) visited[j] = 0;
    visited[o] = 1;
    stack[o] = o;
    int32_t sp = o + 1, seen = 1;
    while (sp > o) {
        const int32_t s = stack[--sp];
        const int32_t cs = vf_corner[s], fs = cs / 3, ks = cs % 3;
        const int32_t w1 = faces[3 * (int64_t)fs + (ks + 1) % 3], w2 = faces[3 * (int64_t)fs + (ks + 2) % 3];
        for (int32_t j = o; j < e; ++j) {
            if (visited[j]) continue;
            const int32_t c = vf_corner[j], fc = c / 3, kc = c % 3;
            const int32_t a = faces[3 * (int64_t)fc + (kc + 1) % 3], b = faces[3 * (int64_t)fc + (kc + 2) % 3];
            if (a == w1 || a == w2 || b == w1 || b == w2) {
                visited[j] = 1;
                stack[sp++] = j;                                   // each corner is pushed once: sp stays below e
                ++seen;
            }
        }
    }
    if (seen < e - o) {
        split[v] = 1;
        atomicAdd(totals, 1ull);
    }
}

// split vertex number r (in the order of its first corner) is split_ids[r]: row V + r of verts <- its position, and every corner of its
// first fan is re-pointed to V + r
__global__ void mc_fan_split_kernel(float* __restrict__ verts, uint32_t V, int32_t* __restrict__ faces, const int32_t* __restrict__ vf_off,
                                    const int32_t* __restrict__ vf_corner, const uint8_t* __restrict__ visited, const int32_t* __restrict__ split_ids,
                                    uint32_t n_split) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_split) return;
    const int32_t v = split_ids[r];
    const int32_t nv = (int32_t)(V + r);
#pragma unroll
    for (int c = 0; c < 3; ++c) verts[3 * (int64_t)nv + c] = verts[3 * (int64_t)v + c];
    for (int32_t j = vf_off[v]; j < vf_off[v + 1]; ++j)
        if (visited[j]) faces[vf_corner[j]] = nv;
}

}  // namespace

extern "C" {

int n2m_mesh_clean_cell_keys(const float* vertices, uint32_t V, double lo_x, double lo_y, double lo_z, double cell, int32_t nx, int32_t ny,
                             int32_t nz, int64_t* keys, void* stream) {
    if (V == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(keys);
    N2M_REQUIRE(cell > 0.0 && nx > 0 && ny > 0 && nz > 0, N2M_EINVAL, "%s: the cell size and the grid dimensions must be > 0", __func__);
    N2M_REQUIRE((double)nx * ny * nz < 2147483647.0, N2M_EINVAL, "%s: the grid has 2^31 - 1 cells or more", __func__);
    mc_cell_keys_kernel<<<grid_of(V), kMcBlock, 0, (hipStream_t)stream>>>(vertices, V, lo_x, lo_y, lo_z, cell, nx, ny, nz, keys);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_clean_merge_round(const float* vertices, uint32_t V, const int32_t* order, const int64_t* keys, const int32_t* cell_offsets,
                               int32_t nx, int32_t ny, int32_t nz, double r2, const int32_t* state_in, int32_t* state_out, int32_t* blocker,
                               uint32_t* undecided, void* stream) {
    N2M_NOTNULL(undecided);
    hipStream_t s = (hipStream_t)stream;
    N2M_HIP(hipMemsetAsync(undecided, 0, sizeof(uint32_t), s));
    if (V == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(order); N2M_NOTNULL(keys); N2M_NOTNULL(cell_offsets); N2M_NOTNULL(state_in); N2M_NOTNULL(state_out);
    N2M_NOTNULL(blocker);
    N2M_REQUIRE(nx > 0 && ny > 0 && nz > 0, N2M_EINVAL, "%s: the grid dimensions must be > 0", __func__);
    mc_merge_round_kernel<<<grid_of(V), kMcBlock, 0, s>>>(vertices, V, order, keys, cell_offsets, nx, ny, nz, r2, state_in, state_out, blocker,
                                                          undecided);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_clean_repoint(int32_t* faces, uint32_t F, const int32_t* dest, uint8_t* face_alive, void* stream) {
    if (F == 0) return 0;
    N2M_NOTNULL(faces); N2M_NOTNULL(dest); N2M_NOTNULL(face_alive);
    mc_repoint_kernel<<<grid_of(F), kMcBlock, 0, (hipStream_t)stream>>>(faces, F, dest, face_alive);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_clean_dup_null(const float* vertices, const int32_t* faces, uint32_t F, const int32_t* order, uint8_t* face_alive, uint64_t* totals,
                            void* stream) {
    N2M_NOTNULL(totals);
    hipStream_t s = (hipStream_t)stream;
    N2M_HIP(hipMemsetAsync(totals, 0, 2 * sizeof(uint64_t), s));
    if (F == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(faces); N2M_NOTNULL(order); N2M_NOTNULL(face_alive);
    mc_dup_null_kernel<<<grid_of(F), kMcBlock, 0, s>>>(vertices, faces, F, order, face_alive, (unsigned long long*)totals);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_clean_components(const float* vertices, const int32_t* faces, uint32_t F, const int32_t* c2e, uint32_t E, void* workspace,
                              uint64_t workspace_bytes, int32_t* label, void* stream) {
    if (F == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(faces); N2M_NOTNULL(c2e); N2M_NOTNULL(workspace); N2M_NOTNULL(label);
    N2M_REQUIRE(workspace_bytes >= 4ull * E + 32ull * F, N2M_EINVAL, "%s: workspace needs 4 bytes per edge and 32 per face", __func__);
    hipStream_t s = (hipStream_t)stream;
    int32_t* rep = (int32_t*)workspace;                        // [E]: the smallest face on the edge
    int32_t* parent = rep + E;                                 // [F]
    int32_t* count = parent + F;                               // [F], per root
    uint32_t* box = (uint32_t*)(count + F);                    // [F][6], per root: encoded lo xyz, hi xyz
    if (E) N2M_HIP(hipMemsetAsync(rep, 0x7f, 4ull * E, s));   // 0x7f7f7f7f: above every face id (3 F < 2^31)
    N2M_HIP(hipMemsetAsync(count, 0, 4ull * F, s));
    N2M_HIP(hipMemsetAsync(box, 0, 24ull * F, s));
    mc_uf_init_kernel<<<grid_of(F), kMcBlock, 0, s>>>(parent, box, F);
    N2M_CHECK_LAUNCH();
    mc_edge_min_face_kernel<<<grid_of(3ull * F), kMcBlock, 0, s>>>(c2e, F, rep);
    N2M_CHECK_LAUNCH();
    mc_union_kernel<<<grid_of(3ull * F), kMcBlock, 0, s>>>(c2e, F, rep, parent);
    N2M_CHECK_LAUNCH();
    mc_component_stats_kernel<<<grid_of(F), kMcBlock, 0, s>>>(vertices, faces, F, parent, label, count, box);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_clean_component_filter(uint32_t F, const int32_t* label, const void* workspace, uint32_t E, int use_diameter, double min_diameter,
                                    int32_t min_faces, uint8_t* face_alive, uint64_t* totals, void* stream) {
    N2M_NOTNULL(totals);
    hipStream_t s = (hipStream_t)stream;
    N2M_HIP(hipMemsetAsync(totals, 0, 5 * sizeof(uint64_t), s));
    if (F == 0) return 0;
    N2M_NOTNULL(label); N2M_NOTNULL(workspace); N2M_NOTNULL(face_alive);
    const int32_t* count = (const int32_t*)workspace + E + F;
    const uint32_t* box = (const uint32_t*)(count + F);
    mc_component_filter_kernel<<<grid_of(F), kMcBlock, 0, s>>>(F, label, count, box, use_diameter, min_diameter, min_faces, face_alive,
                                                               (unsigned long long*)totals);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_clean_nm_edge_init(const float* vertices, const int32_t* faces, uint32_t F, const int32_t* c2e, const int32_t* edge_nf,
                                double* double_area, uint8_t* state, uint64_t* totals, void* stream) {
    N2M_NOTNULL(totals);
    hipStream_t s = (hipStream_t)stream;
    N2M_HIP(hipMemsetAsync(totals, 0, sizeof(uint64_t), s));
    if (F == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(faces); N2M_NOTNULL(c2e); N2M_NOTNULL(edge_nf); N2M_NOTNULL(double_area); N2M_NOTNULL(state);
    mc_nm_edge_init_kernel<<<grid_of(F), kMcBlock, 0, s>>>(vertices, faces, F, c2e, edge_nf, double_area, state, (unsigned long long*)totals);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_clean_nm_edge_round(uint32_t F, const int32_t* c2e, const int32_t* edge_nf, const int32_t* ef_offsets, const int32_t* ef_faces,
                                 const double* double_area, const uint8_t* state_in, uint8_t* state_out, uint64_t* totals, void* stream) {
    N2M_NOTNULL(totals);
    hipStream_t s = (hipStream_t)stream;
    N2M_HIP(hipMemsetAsync(totals, 0, 2 * sizeof(uint64_t), s));
    if (F == 0) return 0;
    N2M_NOTNULL(c2e); N2M_NOTNULL(edge_nf); N2M_NOTNULL(ef_offsets); N2M_NOTNULL(ef_faces); N2M_NOTNULL(double_area); N2M_NOTNULL(state_in);
    N2M_NOTNULL(state_out);
    mc_nm_edge_round_kernel<<<grid_of(F), kMcBlock, 0, s>>>(F, c2e, edge_nf, ef_offsets, ef_faces, double_area, state_in, state_out,
                                                            (unsigned long long*)totals);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_clean_fan_walk(const int32_t* faces, uint32_t F, uint32_t V, const int32_t* vf_offsets, const int32_t* vf_corners, uint8_t* visited,
                            int32_t* stack, uint8_t* split, int32_t* first_corner, uint64_t* totals, void* stream) {
    N2M_NOTNULL(totals);
    hipStream_t s = (hipStream_t)stream;
    N2M_HIP(hipMemsetAsync(totals, 0, sizeof(uint64_t), s));
    if (V == 0) return 0;
    N2M_NOTNULL(vf_offsets); N2M_NOTNULL(split); N2M_NOTNULL(first_corner);
    if (F) { N2M_NOTNULL(faces); N2M_NOTNULL(vf_corners); N2M_NOTNULL(visited); N2M_NOTNULL(stack); }
    mc_fan_walk_kernel<<<grid_of(V), kMcBlock, 0, s>>>(faces, V, vf_offsets, vf_corners, visited, stack, split, first_corner,
                                                       (unsigned long long*)totals);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_clean_fan_split(float* vertices, uint32_t V, int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_corners,
                             const uint8_t* visited, const int32_t* split_ids, uint32_t n_split, void* stream) {
    if (n_split == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(faces); N2M_NOTNULL(vf_offsets); N2M_NOTNULL(vf_corners); N2M_NOTNULL(visited); N2M_NOTNULL(split_ids);
    mc_fan_split_kernel<<<grid_of(n_split), kMcBlock, 0, (hipStream_t)stream>>>(vertices, V, faces, vf_offsets, vf_corners, visited, split_ids,
                                                                                n_split);
    N2M_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
