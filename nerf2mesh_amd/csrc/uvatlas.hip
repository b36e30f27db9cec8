// UV atlas on the device: axis-direction charts, orthographic parametrisation, shelf packing and overlap eviction -- the step the
// reference leaves to xatlas on the host (nerf/renderer.py:312-322).  This is not an xatlas port; the rule is the project's own and is
// stated in DESIGN.md section 4.13.  The passes below are the per-element work; sorting, unique-ing and scans are torch plumbing in
// nerf2mesh_amd/uv_atlas.py, which also drives the packing trials and the eviction rounds.  tests/uv_atlas_ref.py restates the rule
// sequentially in numpy and reproduces every output bit for bit.
//
// Every value that decides an index is an fp64 evaluation of fp32 inputs in a fixed operand order (the library is built without
// fused-multiply-add contraction) or an integer compare.  The atomics are integer min / max / add and union-find hooks, whose results do not
// depend on their order; the one fp64 sum (n2m_uv_sum_f64) runs in a fixed order.  Relaxation rounds read the previous round's labels.
#include <math.h>

#include "n2m_mesh.hpp"

namespace {

constexpr uint32_t kUvBlock = 256;
constexpr int64_t kLaneBox = 64;                // canvas passes: a face whose texel box is larger than this is walked by its whole wave
constexpr double kRectClamp = 1073741824.0;     // ceil(s * extent) is clamped to 2^30 before it becomes an integer

inline uint32_t grid_of(uint64_t n) { return n2m_ceil_div(n, kUvBlock); }

// n . d_k for direction k = 2 * axis + (sign < 0)
__device__ __forceinline__ double dir_dot(const double n[3], int k) { return (k & 1) ? -n[k >> 1] : n[k >> 1]; }

// ------------------------------------------------------------------------------------------------------------ frames, labels, relaxation
// normal [F][3], da [F] = |normal|, elen [F][3] = the length of corner k's edge (v_k, v_k+1), label [F] = argmax_k n . d_k (ties: lowest
// k); totals[0] += faces with a repeated corner or a zero normal
__global__ void uv_frames_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, uint32_t F, double* __restrict__ normal,
                                 double* __restrict__ da, double* __restrict__ elen, int32_t* __restrict__ label,
                                 unsigned long long* __restrict__ totals) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    double n[3];
    face_cross(verts, faces, f, n);
    const double a = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    int32_t v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        normal[3 * (int64_t)f + k] = n[k];
        v[k] = faces[3 * (int64_t)f + k];
    }
    da[f] = a;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t p = v[k], q = v[(k + 1) % 3];
        const double dx = ldc(verts, q, 0) - ldc(verts, p, 0), dy = ldc(verts, q, 1) - ldc(verts, p, 1), dz = ldc(verts, q, 2) - ldc(verts, p, 2);
        elen[3 * (int64_t)f + k] = sqrt((dx * dx + dy * dy) + dz * dz);
    }
    int best = 0;
    double best_val = dir_dot(n, 0);
#pragma unroll
    for (int k = 1; k < 6; ++k) {
        const double val = dir_dot(n, k);
        if (val > best_val) { best_val = val; best = k; }
    }
    label[f] = best;
    if (v[0] == v[1] || v[1] == v[2] || v[2] == v[0] || a == 0.0) atomicAdd(totals, 1ull);
}

// emin / emax [E] <- the smallest / largest face on the edge (on an edge with two faces: the pair)
__global__ void uv_edge_faces_kernel(const int32_t* __restrict__ c2e, uint32_t F, int32_t* __restrict__ emin, int32_t* __restrict__ emax) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3u * F) return;
    const int32_t e = c2e[i];
    atomicMin(emin + e, (int32_t)(i / 3));
    atomicMax(emax + e, (int32_t)(i / 3));
}

// One Jacobi round: per label, the summed lengths (corner order 0, 1, 2) of the edges shared with exactly one other face of that label;
// the candidate is the largest positive sum (ties: lowest k) and is taken if n . d_cand >= min_cos * |n|.
__global__ void uv_relax_kernel(uint32_t F, const int32_t* __restrict__ c2e, const int32_t* __restrict__ nf, const int32_t* __restrict__ emin,
                                const int32_t* __restrict__ emax, const double* __restrict__ elen, const double* __restrict__ normal,
                                const double* __restrict__ da, double min_cos, const int32_t* __restrict__ label_in,
                                int32_t* __restrict__ label_out, unsigned long long* __restrict__ changed) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    double sums[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t e = c2e[3 * (int64_t)f + k];
        if (nf[e] != 2) continue;
        const int32_t l = label_in[emin[e] + emax[e] - (int32_t)f];
        const double len = elen[3 * (int64_t)f + k];
#pragma unroll
        for (int j = 0; j < 6; ++j) sums[j] = (j == l) ? sums[j] + len : sums[j];       // (no dynamic index: the sums stay in registers)
    }
    int cand = 0;
    double best = sums[0];
#pragma unroll
    for (int j = 1; j < 6; ++j)
        if (sums[j] > best) { best = sums[j]; cand = j; }
    const int32_t own = label_in[f];
    int32_t out = own;
    if (best > 0.0 && cand != own) {
        const double n[3] = {normal[3 * (int64_t)f], normal[3 * (int64_t)f + 1], normal[3 * (int64_t)f + 2]};
        if (dir_dot(n, cand) >= min_cos * da[f]) out = cand;
    }
    label_out[f] = out;
    if (out != own) atomicAdd(changed, 1ull);
}

// ------------------------------------------------------------------------------------------------------------ charts
__global__ void uv_parent_init_kernel(int32_t* __restrict__ parent, uint32_t F) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < F) parent[f] = (int32_t)f;
}

// the union-find of the mesh cleaning with an edge filter: exactly two faces, equal label, equal eviction generation
__global__ void uv_union_kernel(const int32_t* __restrict__ c2e, const int32_t* __restrict__ nf, const int32_t* __restrict__ emin,
                                const int32_t* __restrict__ emax, const int32_t* __restrict__ label, const int32_t* __restrict__ gen, uint32_t F,
                                int32_t* parent) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3u * F) return;
    const int32_t e = c2e[i], f = (int32_t)(i / 3);
    if (nf[e] != 2) return;
    const int32_t g = emin[e] + emax[e] - f;
    if (g < f && label[g] == label[f] && gen[g] == gen[f]) uf_unite(parent, f, g);      // (g > f: that face's thread hooks the pair)
}

// root [F] <- the chart's smallest face; is_root [F] <- the face is that face
__global__ void uv_roots_kernel(const int32_t* __restrict__ parent, uint32_t F, int32_t* __restrict__ root, uint8_t* __restrict__ is_root) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    int32_t x = (int32_t)f, p = parent[x];
    while (p != x) { x = p; p = parent[x]; }
    root[f] = x;
    is_root[f] = x == (int32_t)f ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ parametrisation, boxes
// (u axis, v axis) of direction k: the pair that gives a face with n . d_k > 0 a positive UV area
__device__ __forceinline__ void uv_axes(int k, int& iu, int& iv) {
    const int a = k >> 1, b = (a + 1) % 3, c = (a + 2) % 3;
    iu = (k & 1) ? c : b;
    iv = (k & 1) ? b : c;
}

// proj [T][2] <- the UV vertex's mesh vertex projected along its chart's direction; box [C][4] (encoded min u, min v, max u, max v)
__global__ void uv_project_kernel(const float* __restrict__ verts, const int32_t* __restrict__ vmapping, const int32_t* __restrict__ vchart,
                                  const int32_t* __restrict__ chart_label, uint32_t T, float* __restrict__ proj, uint32_t* __restrict__ box) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const int32_t c = vchart[t], v = vmapping[t];
    int iu, iv;
    uv_axes(chart_label[c], iu, iv);
    const float pu = verts[3 * (int64_t)v + iu], pv = verts[3 * (int64_t)v + iv];
    proj[2 * (int64_t)t] = pu;
    proj[2 * (int64_t)t + 1] = pv;
    atomicMin(box + 4 * (int64_t)c, fenc(pu));
    atomicMin(box + 4 * (int64_t)c + 1, fenc(pv));
    atomicMax(box + 4 * (int64_t)c + 2, fenc(pu));
    atomicMax(box + 4 * (int64_t)c + 3, fenc(pv));
}

__global__ void uv_box_init_kernel(uint32_t* __restrict__ box, uint32_t C) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    box[4 * (int64_t)c] = box[4 * (int64_t)c + 1] = 0xffffffffu;
    box[4 * (int64_t)c + 2] = box[4 * (int64_t)c + 3] = 0u;
}

// The fp64 sum in ONE order: thread t adds x[t], x[t + 256], ... in order, thread 0 then adds the 256 partials in order.
__global__ __launch_bounds__(kUvBlock) void uv_sum_kernel(const double* __restrict__ x, uint32_t n, double* __restrict__ out) {
    __shared__ double part[kUvBlock];
    double a = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += kUvBlock) a += x[i];
    part[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (uint32_t t = 0; t < kUvBlock; ++t) s += part[t];
        *out = s;
    }
}

// ------------------------------------------------------------------------------------------------------------ packing
// rect [C][2] <- (width, height) = ceil(s * extent) + 1 + 2 * gutter; key [C] <- -(height * 2^32 + width): a stable ascending sort of
// the keys orders the charts by height descending, width descending, id ascending
__global__ void uv_rects_kernel(const uint32_t* __restrict__ box, uint32_t C, double s, int32_t gutter, int32_t* __restrict__ rect,
                                int64_t* __restrict__ key) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const uint32_t* b = box + 4 * (int64_t)c;
    const double eu = (double)fdec(b[2]) - (double)fdec(b[0]), ev = (double)fdec(b[3]) - (double)fdec(b[1]);
    const int32_t w = (int32_t)fmin(ceil(s * eu), kRectClamp) + 1 + 2 * gutter, h = (int32_t)fmin(ceil(s * ev), kRectClamp) + 1 + 2 * gutter;
    rect[2 * (int64_t)c] = w;
    rect[2 * (int64_t)c + 1] = h;
    key[c] = -(((int64_t)h << 32) + (int64_t)w);
}

// Shelf packing, a serial recurrence over the charts in `order`: one workgroup stages 256 rectangles at a time in LDS, thread 0 runs the
// recurrence on them, all threads write the origins back.  result[0] <- the shelves fit, result[1] <- the height they use.
__global__ __launch_bounds__(kUvBlock) void uv_shelf_pack_kernel(const int32_t* __restrict__ rect, const int32_t* __restrict__ order, uint32_t C,
                                                                 int32_t height, int32_t width, int32_t* __restrict__ origin,
                                                                 int32_t* __restrict__ result) {
    __shared__ int32_t sw[kUvBlock], sh[kUvBlock], sx[kUvBlock], sy[kUvBlock];
    __shared__ int64_t state[3];                      // x, y, shelf height
    __shared__ int32_t fits;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) { state[0] = state[1] = state[2] = 0; fits = 1; }
    for (uint32_t base = 0; base < C; base += kUvBlock) {
        const uint32_t i = base + tid;
        int32_t c = 0;
        if (i < C) {
            c = order[i];
            sw[tid] = rect[2 * (int64_t)c];
            sh[tid] = rect[2 * (int64_t)c + 1];
        }
        __syncthreads();
        if (tid == 0) {
            int64_t x = state[0], y = state[1], shelf = state[2];
            const uint32_t n = C - base < kUvBlock ? C - base : kUvBlock;
            for (uint32_t j = 0; j < n; ++j) {
                const int64_t w = sw[j], h = sh[j];
                if (w > width) fits = 0;
                if (x + w > width) { y += shelf; x = 0; shelf = 0; }
                sx[j] = (int32_t)(x < 0x7fffffff ? x : 0x7fffffff);
                sy[j] = (int32_t)(y < 0x7fffffff ? y : 0x7fffffff);
                x += w;
                shelf = h > shelf ? h : shelf;
            }
            state[0] = x; state[1] = y; state[2] = shelf;
        }
        __syncthreads();
        if (i < C) {
            origin[2 * (int64_t)c] = sx[tid];
            origin[2 * (int64_t)c + 1] = sy[tid];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t used = state[1] + state[2];
        result[0] = (fits && used <= height) ? 1 : 0;
        result[1] = (int32_t)(used < 0x7fffffff ? used : 0x7fffffff);
    }
}

// vt = ((rect origin + gutter + 0.5) + s * (p - chart min)) / (width, height), fp64 rounded once to fp32
__global__ void uv_write_vt_kernel(const float* __restrict__ proj, const int32_t* __restrict__ vchart, const uint32_t* __restrict__ box,
                                   const int32_t* __restrict__ origin, uint32_t T, double s, int32_t gutter, int32_t height, int32_t width,
                                   float* __restrict__ vt) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const int32_t c = vchart[t];
    const double du = (double)proj[2 * (int64_t)t] - (double)fdec(box[4 * (int64_t)c]);
    const double dv = (double)proj[2 * (int64_t)t + 1] - (double)fdec(box[4 * (int64_t)c + 1]);
    const double ox = (double)origin[2 * (int64_t)c], oy = (double)origin[2 * (int64_t)c + 1], g = (double)gutter;
    vt[2 * (int64_t)t] = (float)(((ox + g + 0.5) + s * du) / (double)width);
    vt[2 * (int64_t)t + 1] = (float)(((oy + g + 0.5) + s * dv) / (double)height);
}

// ------------------------------------------------------------------------------------------------------------ overlap canvas
struct UvTri {
    double x[3], y[3];          // corners in texels: the fp32 uv times the resolution, exact in fp64
    int32_t id[3];              // UV-vertex ids
    int32_t x0, x1, y0, y1;     // texel box (clamped to the image) that bounds the walk
    int64_t n;                  // texels in the box
};

__device__ __forceinline__ int32_t texel_bound(double v, int32_t last) {
    v = fmin(fmax(v, 0.0), (double)last);             // (a NaN becomes 0: the walk stays inside the image whatever the input)
    return (int32_t)v;
}

__device__ __forceinline__ void load_tri(const float* __restrict__ vt, const int32_t* __restrict__ ft, uint32_t f, int32_t H, int32_t W, UvTri& t) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t.id[k] = ft[3 * (int64_t)f + k];
        t.x[k] = (double)vt[2 * (int64_t)t.id[k]] * (double)W;
        t.y[k] = (double)vt[2 * (int64_t)t.id[k] + 1] * (double)H;
    }
    const double lox = fmin(fmin(t.x[0], t.x[1]), t.x[2]), hix = fmax(fmax(t.x[0], t.x[1]), t.x[2]);
    const double loy = fmin(fmin(t.y[0], t.y[1]), t.y[2]), hiy = fmax(fmax(t.y[0], t.y[1]), t.y[2]);
    t.x0 = texel_bound(floor(lox - 0.5), W - 1);
    t.x1 = texel_bound(ceil(hix - 0.5), W - 1);
    t.y0 = texel_bound(floor(loy - 0.5), H - 1);
    t.y1 = texel_bound(ceil(hiy - 0.5), H - 1);
    t.n = (t.x1 >= t.x0 && t.y1 >= t.y0) ? (int64_t)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) : 0;
}

// edge function of the directed edge p -> q, evaluated from the endpoint with the smaller UV-vertex id: the two faces of a chart edge get
// values that are exact negatives of each other, so a texel centre is never strictly inside both
__device__ __forceinline__ double edge_fn(const UvTri& t, int p, int q, double px, double py) {
    if (t.id[p] < t.id[q]) return (t.x[q] - t.x[p]) * (py - t.y[p]) - (t.y[q] - t.y[p]) * (px - t.x[p]);
    return -((t.x[p] - t.x[q]) * (py - t.y[q]) - (t.y[p] - t.y[q]) * (px - t.x[q]));
}

// texel `idx` of the face's box: PASS 0 writes the face id with an atomic min if the centre is strictly inside; PASS 1 returns whether such
// a texel holds a lower id
template <int PASS>
__device__ __forceinline__ bool canvas_texel(const UvTri& t, int64_t idx, int32_t f, int32_t W, int32_t* __restrict__ canvas) {
    const int32_t bw = t.x1 - t.x0 + 1;
    const int32_t x = t.x0 + (int32_t)(idx % bw), y = t.y0 + (int32_t)(idx / bw);
    const double px = (double)x + 0.5, py = (double)y + 0.5;
    if (!(edge_fn(t, 0, 1, px, py) > 0.0 && edge_fn(t, 1, 2, px, py) > 0.0 && edge_fn(t, 2, 0, px, py) > 0.0)) return false;
    int32_t* cell = canvas + (int64_t)y * W + x;
    if (PASS == 0) { atomicMin(cell, f); return false; }
    return *cell < f;
}

// One lane per face; a face whose box exceeds kLaneBox texels is walked by all 64 lanes of its wave instead (one such face after the
// other), so that one large face does not hold 63 idle lanes for thousands of iterations.
template <int PASS>
__global__ __launch_bounds__(kUvBlock) void uv_canvas_kernel(const float* __restrict__ vt, const int32_t* __restrict__ ft, uint32_t F, int32_t H,
                                                             int32_t W, int32_t* __restrict__ canvas, uint8_t* __restrict__ evicted) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = f < F;
    const int lane = threadIdx.x & (N2M_WAVE - 1);
    UvTri t;
    t.n = 0;
    if (valid) load_tri(vt, ft, f, H, W, t);
    const bool big = t.n > kLaneBox;
    if (valid && !big) {
        bool hit = false;
        for (int64_t i = 0; i < t.n; ++i) hit |= canvas_texel<PASS>(t, i, (int32_t)f, W, canvas);
        if (PASS == 1 && hit) evicted[f] = 1;
    }
    unsigned long long todo = __ballot(big);           // wave-uniform from here on: every lane takes part in every big face
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1;
        const uint32_t fb = (uint32_t)__shfl((int)f, src);
        UvTri b;
        load_tri(vt, ft, fb, H, W, b);
        bool hit = false;
        for (int64_t i = lane; i < b.n; i += N2M_WAVE) hit |= canvas_texel<PASS>(b, i, (int32_t)fb, W, canvas);
        if (PASS == 1 && hit) evicted[fb] = 1;         // (several lanes may store the same 1)
    }
}

// area [F] <- the signed UV area in texels, density [F] <- area / (da / 2)
__global__ void uv_metrics_kernel(const float* __restrict__ vt, const int32_t* __restrict__ ft, const double* __restrict__ da, uint32_t F, int32_t H,
                                  int32_t W, double* __restrict__ area, double* __restrict__ density) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    double x[3], y[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t id = ft[3 * (int64_t)f + k];
        x[k] = (double)vt[2 * (int64_t)id] * (double)W;
        y[k] = (double)vt[2 * (int64_t)id + 1] * (double)H;
    }
    const double a = 0.5 * ((x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0]));
    area[f] = a;
    density[f] = a / (0.5 * da[f]);
}

}  // namespace

extern "C" {

int n2m_uv_face_frames(const float* vertices, const int32_t* faces, uint32_t F, double* normal, double* double_area, double* edge_length,
                       int32_t* label, uint64_t* totals, void* stream) {
    N2M_NOTNULL(totals);
    hipStream_t s = (hipStream_t)stream;
    N2M_HIP(hipMemsetAsync(totals, 0, sizeof(uint64_t), s));
    if (F == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(faces); N2M_NOTNULL(normal); N2M_NOTNULL(double_area); N2M_NOTNULL(edge_length); N2M_NOTNULL(label);
    uv_frames_kernel<<<grid_of(F), kUvBlock, 0, s>>>(vertices, faces, F, normal, double_area, edge_length, label, (unsigned long long*)totals);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_uv_edge_faces(const int32_t* c2e, uint32_t F, uint32_t E, int32_t* edge_min_face, int32_t* edge_max_face, void* stream) {
    if (F == 0 || E == 0) return 0;
    N2M_NOTNULL(c2e); N2M_NOTNULL(edge_min_face); N2M_NOTNULL(edge_max_face);
    hipStream_t s = (hipStream_t)stream;
    N2M_HIP(hipMemsetAsync(edge_min_face, 0x7f, 4ull * E, s));      // 0x7f7f7f7f: above every face id (3 F < 2^31)
    N2M_HIP(hipMemsetAsync(edge_max_face, 0xff, 4ull * E, s));      // -1
    uv_edge_faces_kernel<<<grid_of(3ull * F), kUvBlock, 0, s>>>(c2e, F, edge_min_face, edge_max_face);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_uv_relax_round(uint32_t F, const int32_t* c2e, const int32_t* edge_nf, const int32_t* edge_min_face, const int32_t* edge_max_face,
                       const double* edge_length, const double* normal, const double* double_area, double min_cos, const int32_t* label_in,
                       int32_t* label_out, uint64_t* changed, void* stream) {
    N2M_NOTNULL(changed);
    hipStream_t s = (hipStream_t)stream;
    N2M_HIP(hipMemsetAsync(changed, 0, sizeof(uint64_t), s));
    if (F == 0) return 0;
    N2M_NOTNULL(c2e); N2M_NOTNULL(edge_nf); N2M_NOTNULL(edge_min_face); N2M_NOTNULL(edge_max_face); N2M_NOTNULL(edge_length); N2M_NOTNULL(normal);
    N2M_NOTNULL(double_area); N2M_NOTNULL(label_in); N2M_NOTNULL(label_out);
    N2M_REQUIRE(min_cos > 0.0 && min_cos <= 1.0, N2M_EINVAL, "%s: min_cos must lie in (0, 1]", __func__);
    N2M_REQUIRE(label_in != label_out, N2M_EINVAL, "%s: a round reads one label buffer and writes another", __func__);
    uv_relax_kernel<<<grid_of(F), kUvBlock, 0, s>>>(F, c2e, edge_nf, edge_min_face, edge_max_face, edge_length, normal, double_area, min_cos,
                                                    label_in, label_out, (unsigned long long*)changed);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_uv_charts(uint32_t F, const int32_t* c2e, const int32_t* edge_nf, const int32_t* edge_min_face, const int32_t* edge_max_face,
                  const int32_t* label, const int32_t* generation, int32_t* parent, int32_t* root, uint8_t* is_root, void* stream) {
    if (F == 0) return 0;
    N2M_NOTNULL(c2e); N2M_NOTNULL(edge_nf); N2M_NOTNULL(edge_min_face); N2M_NOTNULL(edge_max_face); N2M_NOTNULL(label); N2M_NOTNULL(generation);
    N2M_NOTNULL(parent); N2M_NOTNULL(root); N2M_NOTNULL(is_root);
    hipStream_t s = (hipStream_t)stream;
    uv_parent_init_kernel<<<grid_of(F), kUvBlock, 0, s>>>(parent, F);
    N2M_CHECK_LAUNCH();
    uv_union_kernel<<<grid_of(3ull * F), kUvBlock, 0, s>>>(c2e, edge_nf, edge_min_face, edge_max_face, label, generation, F, parent);
    N2M_CHECK_LAUNCH();
    uv_roots_kernel<<<grid_of(F), kUvBlock, 0, s>>>(parent, F, root, is_root);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_uv_project(const float* vertices, const int32_t* vmapping, const int32_t* vertex_chart, const int32_t* chart_label, uint32_t T, uint32_t C,
                   float* projected, uint32_t* chart_box, void* stream) {
    if (T == 0 || C == 0) return 0;
    N2M_NOTNULL(vertices); N2M_NOTNULL(vmapping); N2M_NOTNULL(vertex_chart); N2M_NOTNULL(chart_label); N2M_NOTNULL(projected); N2M_NOTNULL(chart_box);
    hipStream_t s = (hipStream_t)stream;
    uv_box_init_kernel<<<grid_of(C), kUvBlock, 0, s>>>(chart_box, C);
    N2M_CHECK_LAUNCH();
    uv_project_kernel<<<grid_of(T), kUvBlock, 0, s>>>(vertices, vmapping, vertex_chart, chart_label, T, projected, chart_box);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_uv_sum_f64(const double* values, uint32_t n, double* sum, void* stream) {
    N2M_NOTNULL(sum);
    if (n) N2M_NOTNULL(values);
    uv_sum_kernel<<<1, kUvBlock, 0, (hipStream_t)stream>>>(values, n, sum);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_uv_rects(const uint32_t* chart_box, uint32_t C, double scale, int32_t gutter, int32_t* rect, int64_t* sort_key, void* stream) {
    if (C == 0) return 0;
    N2M_NOTNULL(chart_box); N2M_NOTNULL(rect); N2M_NOTNULL(sort_key);
    N2M_REQUIRE(scale > 0.0 && gutter >= 0 && gutter < (1 << 20), N2M_EINVAL, "%s: the scale must be > 0 and the gutter in [0, 2^20)", __func__);
    uv_rects_kernel<<<grid_of(C), kUvBlock, 0, (hipStream_t)stream>>>(chart_box, C, scale, gutter, rect, sort_key);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_uv_shelf_pack(const int32_t* rect, const int32_t* order, uint32_t C, int32_t height, int32_t width, int32_t* origin, int32_t* result,
                      void* stream) {
    N2M_NOTNULL(result);
    N2M_REQUIRE(height > 0 && width > 0, N2M_EINVAL, "%s: the resolution must be > 0", __func__);
    if (C) { N2M_NOTNULL(rect); N2M_NOTNULL(order); N2M_NOTNULL(origin); }
    uv_shelf_pack_kernel<<<1, kUvBlock, 0, (hipStream_t)stream>>>(rect, order, C, height, width, origin, result);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_uv_write_vt(const float* projected, const int32_t* vertex_chart, const uint32_t* chart_box, const int32_t* origin, uint32_t T, double scale,
                    int32_t gutter, int32_t height, int32_t width, float* vt, void* stream) {
    if (T == 0) return 0;
    N2M_NOTNULL(projected); N2M_NOTNULL(vertex_chart); N2M_NOTNULL(chart_box); N2M_NOTNULL(origin); N2M_NOTNULL(vt);
    N2M_REQUIRE(height > 0 && width > 0 && gutter >= 0, N2M_EINVAL, "%s: the resolution must be > 0 and the gutter >= 0", __func__);
    uv_write_vt_kernel<<<grid_of(T), kUvBlock, 0, (hipStream_t)stream>>>(projected, vertex_chart, chart_box, origin, T, scale, gutter, height, width,
                                                                         vt);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_uv_canvas_evict(const float* vt, const int32_t* ft, uint32_t F, int32_t height, int32_t width, int32_t* canvas, uint8_t* evicted,
                        void* stream) {
    if (F == 0) return 0;
    N2M_NOTNULL(vt); N2M_NOTNULL(ft); N2M_NOTNULL(canvas); N2M_NOTNULL(evicted);
    N2M_REQUIRE(height > 0 && width > 0 && (int64_t)height * width < (1ll << 31), N2M_EINVAL, "%s: the canvas needs 0 < height * width < 2^31",
                __func__);
    hipStream_t s = (hipStream_t)stream;
    N2M_HIP(hipMemsetAsync(canvas, 0x7f, 4ull * height * width, s));   // above every face id
    N2M_HIP(hipMemsetAsync(evicted, 0, F, s));
    uv_canvas_kernel<0><<<grid_of(F), kUvBlock, 0, s>>>(vt, ft, F, height, width, canvas, evicted);
    N2M_CHECK_LAUNCH();
    uv_canvas_kernel<1><<<grid_of(F), kUvBlock, 0, s>>>(vt, ft, F, height, width, canvas, evicted);
    N2M_CHECK_LAUNCH();
    return 0;
}

int n2m_uv_face_metrics(const float* vt, const int32_t* ft, const double* double_area, uint32_t F, int32_t height, int32_t width, double* texel_area,
                        double* density, void* stream) {
    if (F == 0) return 0;
    N2M_NOTNULL(vt); N2M_NOTNULL(ft); N2M_NOTNULL(double_area); N2M_NOTNULL(texel_area); N2M_NOTNULL(density);
    uv_metrics_kernel<<<grid_of(F), kUvBlock, 0, (hipStream_t)stream>>>(vt, ft, double_area, F, height, width, texel_area, density);
    N2M_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
