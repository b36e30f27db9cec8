// Closest-point queries on a triangle mesh: a linear bounding-volume hierarchy (Karras 2012, "Maximizing parallelism in the construction
// of BVHs, octrees, and k-d trees") built on the device, and its traversal.  Driven by nerf2mesh_amd/mesh_query.py; the rule, and why the
// traversal returns what the exhaustive scan returns bit for bit, are in DESIGN.md section 4.15; tests/mesh_query_ref.py restates the
// scan in numpy.
//
// n = the number of indexed faces (the faces with three distinct vertex indices).  Node ids: internal nodes 0 .. n - 2 (0 is the root),
// leaf j (the face leaf_face[j], j-th in key order) is node n - 1 + j; with n == 1 the only node, 0, is that leaf.  children [n - 1][2]
// i32, parent [2n - 1] i32 (-1 at the root), boxes [2n - 1][6] f32 = min xyz, max xyz of the fp32 vertex coordinates below the node:
// min and max are exact, so a box does not depend on the order its children arrived in.
//
// The query's distances are fp64 + - * / only (-ffp-contract=off); the boxes only ever decide what is skipped.
#include <math.h>

#include "n2m_common.hpp"
#include "n2m_mesh.hpp"

namespace {

constexpr uint32_t kMqBlock = 256;
constexpr uint32_t kMqWave = 64;        // the traversal's workgroup: one wave
constexpr int kMqStack = 64;            // unique keys below 2^62: a node's common prefix grows by a bit per level, so depth <= 62
constexpr int64_t kMqNoKey = INT64_MAX;

__device__ __forceinline__ D3 ldv(const float* __restrict__ v, int32_t i) {
    return D3{(double)v[3 * (int64_t)i], (double)v[3 * (int64_t)i + 1], (double)v[3 * (int64_t)i + 2]};
}

// cell 0 .. 1023 of x along one axis; a NaN goes to cell 0
__device__ __forceinline__ uint32_t mq_cell(double x, double lo, double scale) {
    const double q = (x - lo) * scale;
    if (!(q >= 0.0)) return 0u;
    return q < 1023.0 ? (uint32_t)q : 1023u;
}

// ------------------------------------------------------------------------------------------------------------ keys
__global__ void mq_morton_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, uint32_t F, double lox, double loy, double loz,
                                 double sx, double sy, double sz, int64_t* __restrict__ keys) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int32_t a = faces[3 * (int64_t)f], b = faces[3 * (int64_t)f + 1], c = faces[3 * (int64_t)f + 2];
    if (a == b || b == c || c == a) { keys[f] = kMqNoKey; return; }
    const D3 s = add(add(ldv(verts, a), ldv(verts, b)), ldv(verts, c));
    const uint32_t code = n2m_morton(mq_cell(s.x / 3.0, lox, sx), mq_cell(s.y / 3.0, loy, sy), mq_cell(s.z / 3.0, loz, sz));
    keys[f] = (int64_t)(((uint64_t)code << 32) | (uint64_t)f);
}

// ------------------------------------------------------------------------------------------------------------ hierarchy
// length of the common prefix of keys i and j, -1 outside the array (the keys are unique: no tie to break)
__device__ __forceinline__ int mq_delta(const uint64_t* __restrict__ keys, int64_t n, int64_t i, int64_t j) {
    if (j < 0 || j >= n) return -1;
    return __clzll((long long)(keys[i] ^ keys[j]));
}

__global__ void mq_hierarchy_kernel(const uint64_t* __restrict__ keys, uint32_t n_, int32_t* __restrict__ children, int32_t* __restrict__ parent) {
    const int64_t n = n_;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) parent[0] = -1;
    if (i >= n - 1) return;
    const int64_t d = mq_delta(keys, n, i, i + 1) > mq_delta(keys, n, i, i - 1) ? 1 : -1;
    const int dmin = mq_delta(keys, n, i, i - d);
    int64_t lmax = 2;
    while (mq_delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (mq_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = mq_delta(keys, n, i, j);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (mq_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int64_t gamma = i + s * d + (d < 0 ? -1 : 0);
    const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
    const int32_t left = (int32_t)(lo == gamma ? n - 1 + gamma : gamma), right = (int32_t)(hi == gamma + 1 ? n - 1 + gamma + 1 : gamma + 1);
    children[2 * i] = left;
    children[2 * i + 1] = right;
    parent[left] = (int32_t)i;
    parent[right] = (int32_t)i;
}

// ------------------------------------------------------------------------------------------------------------ boxes
// A box that another workgroup reads is stored and loaded with agent-scope atomics (never a cached plain access), and the arrival counter
// orders the two: store, fence, add on the first arriver; add, fence, load on the second.
__device__ __forceinline__ void mq_store_box(float* boxes, int64_t node, const float b[6]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) __hip_atomic_store(boxes + 6 * node + k, b[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void mq_refit_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, const int32_t* __restrict__ leaf_face, uint32_t n,
                                const int32_t* __restrict__ children, const int32_t* __restrict__ parent, float* boxes, int32_t* counters) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t* t = faces + 3 * (int64_t)leaf_face[j];
    float b[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float x = verts[3 * (int64_t)t[0] + k], y = verts[3 * (int64_t)t[1] + k], z = verts[3 * (int64_t)t[2] + k];
        b[k] = fminf(fminf(x, y), z);
        b[3 + k] = fmaxf(fmaxf(x, y), z);
    }
    int32_t node = (int32_t)(n - 1 + j);
    mq_store_box(boxes, node, b);
    while (true) {
        const int32_t p = parent[node];
        if (p < 0) return;
        __threadfence();
        if (atomicAdd(counters + p, 1) == 0) return;             // the first arriver leaves; the second one forms the box
        __threadfence();
        const int32_t sib = children[2 * (int64_t)p] ^ children[2 * (int64_t)p + 1] ^ node;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            b[k] = fminf(b[k], __hip_atomic_load(boxes + 6 * (int64_t)sib + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            b[3 + k] = fmaxf(b[3 + k], __hip_atomic_load(boxes + 6 * (int64_t)sib + 3 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
        node = p;
        mq_store_box(boxes, node, b);
    }
}

// ------------------------------------------------------------------------------------------------------------ traversal
// squared distance (fp64) from p to the box of `node`: a lower bound, up to its own rounding, of the distance to anything inside
__device__ __forceinline__ double mq_box_d2(const float* __restrict__ boxes, int32_t node, D3 p) {
    const float* b = boxes + 6 * (int64_t)node;
    const double dx = fmax(fmax((double)b[0] - p.x, p.x - (double)b[3]), 0.0);
    const double dy = fmax(fmax((double)b[1] - p.y, p.y - (double)b[4]), 0.0);
    const double dz = fmax(fmax((double)b[2] - p.z, p.z - (double)b[5]), 0.0);
    return dx * dx + dy * dy + dz * dz;
}

// One thread per query, near child first.  The stack of node ids is in the LDS, entry [level][lane]: the lanes of a wave sit at different
// levels, and this layout keeps lane l on bank l mod 32 whatever its level, so a push or a pop is conflict-free; a private array indexed
// at run time would live in scratch memory instead.  16 KiB per wave.
__global__ __launch_bounds__(kMqWave) void mq_closest_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                             const int32_t* __restrict__ leaf_face, uint32_t n_, const int32_t* __restrict__ children,
                                                             const float* __restrict__ boxes, const double* __restrict__ points, uint32_t N, int prune,
                                                             double slack_abs, double slack_rel, double* __restrict__ d2_out,
                                                             int32_t* __restrict__ face_out, double* __restrict__ point_out) {
    __shared__ int32_t stack[kMqStack][kMqWave];
    const uint32_t lane = threadIdx.x;
    const uint32_t q = blockIdx.x * kMqWave + lane;
    if (q >= N) return;                                          // no barrier below
    const int32_t n = (int32_t)n_;
    const D3 p = D3{points[3 * (int64_t)q], points[3 * (int64_t)q + 1], points[3 * (int64_t)q + 2]};
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    double best = INFINITY;
    int32_t best_f = -1;
    D3 best_c = D3{qnan, qnan, qnan};
    int sp = 0;
    bool overflow = false;
    int32_t node = n > 0 ? 0 : -1;
    while (true) {
        // a subtree is skipped only if its box is further than the best distance by more than the slack: strictly, so a tie is visited
        const double limit = best + (slack_abs + slack_rel * best);
        if (node < 0) {
            if (sp == 0) break;
            node = stack[--sp][lane];
            if (prune && mq_box_d2(boxes, node, p) > limit) node = -1;      // the best distance may have fallen since the push
            continue;
        }
        if (node >= n - 1) {
            const int32_t f = leaf_face[node - (n - 1)];
            const int32_t* t = faces + 3 * (int64_t)f;
            const D3 c = closest_on_triangle(p, ldv(verts, t[0]), ldv(verts, t[1]), ldv(verts, t[2]));
            const D3 d = sub(c, p);
            const double dd = dot(d, d);
            if (dd < best || (dd == best && f < best_f)) { best = dd; best_f = f; best_c = c; }
            node = -1;
            continue;
        }
        const int32_t l = children[2 * (int64_t)node], r = children[2 * (int64_t)node + 1];
        const double dl = mq_box_d2(boxes, l, p), dr = mq_box_d2(boxes, r, p);
        const bool vl = !prune || !(dl > limit), vr = !prune || !(dr > limit);
        if (vl && vr) {
            const bool left_first = dl <= dr;
            if (sp < kMqStack) stack[sp++][lane] = left_first ? r : l;
            else overflow = true;                                // not a hierarchy of n2m_mesh_bvh_hierarchy: reported, never written past
            node = left_first ? l : r;
        } else {
            node = vl ? l : (vr ? r : -1);
        }
    }
    if (overflow) { best = qnan; best_f = -2; best_c = D3{qnan, qnan, qnan}; }
    d2_out[q] = best;
    face_out[q] = best_f;
    point_out[3 * (int64_t)q] = best_c.x; point_out[3 * (int64_t)q + 1] = best_c.y; point_out[3 * (int64_t)q + 2] = best_c.z;
}

inline uint32_t grid_of(uint64_t n) { return n2m_ceil_div(n, kMqBlock); }

}  // namespace

extern "C" {

int n2m_mesh_bvh_morton(const float* vertices, const int32_t* faces, uint32_t F, double lo_x, double lo_y, double lo_z, double scale_x,
                        double scale_y, double scale_z, int64_t* keys, void* stream) {
    if (F == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(faces); N2M_NOTNULL(keys);
    N2M_REQUIRE((uint64_t)F * 3 < (1ull << 31), N2M_EINVAL, "%s: %u faces exceed the 31-bit corner ids", __func__, F);
    mq_morton_kernel<<<grid_of(F), kMqBlock, 0, (hipStream_t)stream>>>(vertices, faces, F, lo_x, lo_y, lo_z, scale_x, scale_y, scale_z, keys);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_bvh_hierarchy(const uint64_t* keys, uint32_t n, int32_t* children, int32_t* parent, void* stream) {
    if (n == 0) return 0;
    N2M_NOTNULL(keys); N2M_NOTNULL(parent);
    N2M_REQUIRE(n < (1u << 30), N2M_EINVAL, "%s: %u leaves exceed the 31-bit node ids", __func__, n);
    if (n > 1) N2M_NOTNULL(children);
    mq_hierarchy_kernel<<<grid_of(n > 1 ? n - 1 : 1), kMqBlock, 0, (hipStream_t)stream>>>(keys, n, children, parent);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_bvh_refit(const float* vertices, const int32_t* faces, const int32_t* leaf_face, uint32_t n, const int32_t* children,
                       const int32_t* parent, float* boxes, int32_t* counters, void* stream) {
    if (n == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(faces); N2M_NOTNULL(leaf_face); N2M_NOTNULL(parent); N2M_NOTNULL(boxes);
    N2M_REQUIRE(n < (1u << 30), N2M_EINVAL, "%s: %u leaves exceed the 31-bit node ids", __func__, n);
    hipStream_t s = (hipStream_t)stream;
    if (n > 1) {
        N2M_NOTNULL(children); N2M_NOTNULL(counters);
        N2M_HIP(hipMemsetAsync(counters, 0, (size_t)(n - 1) * sizeof(int32_t), s));
    }
    mq_refit_kernel<<<grid_of(n), kMqBlock, 0, s>>>(vertices, faces, leaf_face, n, children, parent, boxes, counters);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_mesh_closest(const float* vertices, const int32_t* faces, const int32_t* leaf_face, uint32_t n, const int32_t* children, const float* boxes,
                     const double* points, uint32_t N, int prune, double slack_abs, double slack_rel, double* d2, int32_t* face, double* point,
                     void* stream) {
    if (N == 0) return 0;
    N2M_NOTNULL(points); N2M_NOTNULL(d2); N2M_NOTNULL(face); N2M_NOTNULL(point);
    N2M_REQUIRE(n < (1u << 30), N2M_EINVAL, "%s: %u leaves exceed the 31-bit node ids", __func__, n);
    N2M_REQUIRE(prune == 0 || prune == 1, N2M_EINVAL, "%s: prune must be 0 (visit every leaf) or 1, got %d", __func__, prune);
    if (n > 0) { N2M_NOTNULL(vertices); N2M_NOTNULL(faces); N2M_NOTNULL(leaf_face); N2M_NOTNULL(boxes); }
    if (n > 1) N2M_NOTNULL(children);
    mq_closest_kernel<<<n2m_ceil_div(N, kMqWave), kMqWave, 0, (hipStream_t)stream>>>(vertices, faces, leaf_face, n, children, boxes, points, N, prune,
                                                                                    slack_abs, slack_rel, d2, face, point);
    N2M_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
