// The exported asset's fragment shader on the device (reference: renderer.html:424-472): what a viewer computes per fragment from
// mesh_{cas}.obj, feat0_{cas}.jpg, feat1_{cas}.jpg and mlp.json --
//     rgb = clamp(diffuse texel + sigmoid(W1 relu(W0 [view dir, specular texel])), 0, 1)
// -- for every pixel of a view the project's own rasteriser has resolved (rast: barycentrics, z/w, face id + 1).  One thread per pixel,
// one launch per view.  Conventions (include/n2m_hip.h states them in full): the uv of vt is the bake's -- texel (row y, column x) has its
// centre at ((x + .5) / Wt, (y + .5) / Ht), the row index grows with v --, nearest = floor, linear = the four texels around
// (u Wt - .5, v Ht - .5) clamped at the border.
//
// The 288 weights are the same for every lane: they are read through a `const __restrict__` kernel-argument pointer at compile-time
// offsets, which the compiler turns into scalar loads (SGPR operands of the v_fmac chain; no LDS, no per-lane weight traffic).  The hidden
// layer is never materialised: each of its 32 units is folded into the three outputs as soon as it is computed, so the MLP lives in
// ~12 VGPRs.  The cascade table arrives by value in the kernel arguments and is scanned with compile-time indices (selects, not a
// per-lane indexed copy: that would go to scratch).  Mode and filter are template parameters: six straight-line kernels.
#include "n2m_common.hpp"

namespace {

constexpr int HID = 32, NIN = 6;

struct Texel { float r, g, b; };

__device__ __forceinline__ Texel texel_at(const uint8_t* __restrict__ tex, uint32_t Wt, int row, int col) {
    const uint8_t* __restrict__ p = tex + ((size_t)row * Wt + (uint32_t)col) * 3u;
    return Texel{(float)p[0], (float)p[1], (float)p[2]};
}

template <int FILTER>
__device__ __forceinline__ Texel fetch(const uint8_t* __restrict__ tex, uint32_t Ht, uint32_t Wt, float u, float v) {
    const float x = u * (float)Wt, y = v * (float)Ht;
    const int wmax = (int)Wt - 1, hmax = (int)Ht - 1;
    Texel t;
    // (clamped as floats, before the int conversion: a uv far outside [0, 1], or a NaN, still names a texel of the image)
    if (FILTER == N2M_ASSET_NEAREST) {
        const int col = (int)n2m_clampf(floorf(x), 0.0f, (float)wmax), row = (int)n2m_clampf(floorf(y), 0.0f, (float)hmax);
        t = texel_at(tex, Wt, row, col);
    } else {
        const float xs = x - 0.5f, ys = y - 0.5f, x0f = floorf(xs), y0f = floorf(ys);
        const float fx = xs - x0f, fy = ys - y0f;
        const int x0 = (int)n2m_clampf(x0f, -1.0f, (float)wmax), y0 = (int)n2m_clampf(y0f, -1.0f, (float)hmax);
        const int c0 = max(x0, 0), c1 = min(x0 + 1, wmax), r0 = max(y0, 0), r1 = min(y0 + 1, hmax);
        const Texel a = texel_at(tex, Wt, r0, c0), b = texel_at(tex, Wt, r0, c1), c = texel_at(tex, Wt, r1, c0), d = texel_at(tex, Wt, r1, c1);
        const float w00 = (1.0f - fx) * (1.0f - fy), w01 = fx * (1.0f - fy), w10 = (1.0f - fx) * fy, w11 = fx * fy;
        t.r = w00 * a.r + w01 * b.r + w10 * c.r + w11 * d.r;
        t.g = w00 * a.g + w01 * b.g + w10 * c.g + w11 * d.g;
        t.b = w00 * a.b + w01 * b.b + w10 * c.b + w11 * d.b;
    }
    const float s = 1.0f / 255.0f;
    return Texel{t.r * s, t.g * s, t.b * s};
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + __expf(-x)); }

template <int MODE, int FILTER>
__global__ void __launch_bounds__(256)
asset_shade_kernel(const float4* __restrict__ rast, const int32_t* __restrict__ ft, const float* __restrict__ vt,
                   const float* __restrict__ rays_d, const N2mAssetTable tab, const float* __restrict__ w0, const float* __restrict__ w1,
                   uint32_t F, uint32_t T, uint32_t H, uint32_t W, float* __restrict__ rgb) {
    const uint32_t px = blockIdx.x * 64u + (threadIdx.x & 63u), py = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (px >= W || py >= H) return;
    const size_t pix = (size_t)py * W + px;
    float* __restrict__ out = rgb + pix * 3;
    const float4 r = rast[pix];
    const int32_t face = (int32_t)r.w - 1;
    bool ok = face >= 0 && (uint32_t)face < F;
    int32_t i0 = 0, i1 = 0, i2 = 0;
    if (ok) {
        i0 = ft[(size_t)face * 3]; i1 = ft[(size_t)face * 3 + 1]; i2 = ft[(size_t)face * 3 + 2];
        ok = (uint32_t)i0 < T && (uint32_t)i1 < T && (uint32_t)i2 < T;
    }
    if (!ok) { out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f; return; }
    // cascade of the face: the last one whose first face is not above it (compile-time indices into the by-value table)
    const uint8_t* __restrict__ t0 = tab.feat0[0];
    const uint8_t* __restrict__ t1 = tab.feat1[0];
    uint32_t Ht = tab.Ht[0], Wt = tab.Wt[0];
#pragma unroll
    for (int c = 1; c < N2M_ASSET_MAX; ++c) {
        if ((uint32_t)c < tab.count && (uint32_t)face >= tab.face_begin[c]) { t0 = tab.feat0[c]; t1 = tab.feat1[c]; Ht = tab.Ht[c]; Wt = tab.Wt[c]; }
    }
    const float b0 = r.x, b1 = r.y, b2 = 1.0f - r.x - r.y;
    const float u = b0 * vt[2 * (size_t)i0] + b1 * vt[2 * (size_t)i1] + b2 * vt[2 * (size_t)i2];
    const float v = b0 * vt[2 * (size_t)i0 + 1] + b1 * vt[2 * (size_t)i1 + 1] + b2 * vt[2 * (size_t)i2 + 1];
    Texel dif{0.0f, 0.0f, 0.0f};
    if (MODE != N2M_ASSET_SPECULAR) dif = fetch<FILTER>(t0, Ht, Wt, u, v);
    if (MODE == N2M_ASSET_DIFFUSE) { out[0] = dif.r; out[1] = dif.g; out[2] = dif.b; return; }
    const Texel sf = fetch<FILTER>(t1, Ht, Wt, u, v);
    const float dx = rays_d[pix * 3], dy = rays_d[pix * 3 + 1], dz = rays_d[pix * 3 + 2];
    const float inv = rsqrtf(fmaxf(dx * dx + dy * dy + dz * dz, 1e-20f));
    const float in[NIN] = {dx * inv, dy * inv, dz * inv, sf.r, sf.g, sf.b};
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
#pragma unroll
    for (int j = 0; j < HID; ++j) {
        float h = 0.0f;
#pragma unroll
        for (int k = 0; k < NIN; ++k) h = fmaf(w0[j * NIN + k], in[k], h);
        h = fmaxf(h, 0.0f);
        o0 = fmaf(w1[j], h, o0); o1 = fmaf(w1[HID + j], h, o1); o2 = fmaf(w1[2 * HID + j], h, o2);
    }
    float c0 = sigmoidf(o0), c1 = sigmoidf(o1), c2 = sigmoidf(o2);
    if (MODE == N2M_ASSET_FULL) { c0 = n2m_clampf(dif.r + c0, 0.0f, 1.0f); c1 = n2m_clampf(dif.g + c1, 0.0f, 1.0f); c2 = n2m_clampf(dif.b + c2, 0.0f, 1.0f); }
    out[0] = c0; out[1] = c1; out[2] = c2;
}

}  // namespace

extern "C" int n2m_asset_shade(const float* rast, const int32_t* ft, const float* vt, const float* rays_d, const N2mAssetTable* table,
                               const float* w0, const float* w1, uint32_t F, uint32_t T, uint32_t H, uint32_t W, int mode, int filter,
                               float* rgb, void* stream) {
    N2M_REQUIRE(rast != nullptr && ft != nullptr && vt != nullptr && rays_d != nullptr && table != nullptr && w0 != nullptr && w1 != nullptr
                && rgb != nullptr, N2M_ENULL, "asset_shade: NULL rast / ft / vt / rays_d / table / w0 / w1 / rgb");
    N2M_REQUIRE(mode >= N2M_ASSET_FULL && mode <= N2M_ASSET_SPECULAR, N2M_EINVAL, "asset_shade: mode must be 0 (full), 1 (diffuse) or 2 (specular)");
    N2M_REQUIRE(filter == N2M_ASSET_NEAREST || filter == N2M_ASSET_LINEAR, N2M_EINVAL, "asset_shade: filter must be 0 (nearest) or 1 (linear)");
    N2M_REQUIRE(H > 0 && W > 0 && F > 0 && T > 0 && F < (1u << 24), N2M_EINVAL, "asset_shade: H, W, F, T > 0 and F < 2^24 (face ids travel as floats)");
    N2M_REQUIRE(table->count >= 1 && table->count <= N2M_ASSET_MAX, N2M_EINVAL, "asset_shade: 1..8 cascades");
    for (uint32_t c = 0; c < table->count; ++c) {
        N2M_REQUIRE(table->feat0[c] != nullptr && table->feat1[c] != nullptr, N2M_ENULL, "asset_shade: NULL texture of cascade %u", c);
        N2M_REQUIRE(table->Ht[c] > 0 && table->Wt[c] > 0 && table->Ht[c] <= 32768 && table->Wt[c] <= 32768, N2M_EINVAL,
                    "asset_shade: texture of cascade %u must be 1..32768 texels a side", c);
        N2M_REQUIRE(c == 0 ? table->face_begin[0] == 0 : table->face_begin[c] >= table->face_begin[c - 1], N2M_EINVAL,
                    "asset_shade: face_begin must start at 0 and ascend");
    }
    const dim3 grid(n2m_ceil_div(W, 64), n2m_ceil_div(H, 4));
    const hipStream_t s = (hipStream_t)stream;
    const float4* r4 = (const float4*)rast;
#define N2M_ASSET_LAUNCH(M, FL) asset_shade_kernel<M, FL><<<grid, 256, 0, s>>>(r4, ft, vt, rays_d, *table, w0, w1, F, T, H, W, rgb)
    if (filter == N2M_ASSET_NEAREST) {
        if (mode == N2M_ASSET_FULL) N2M_ASSET_LAUNCH(N2M_ASSET_FULL, N2M_ASSET_NEAREST);
        else if (mode == N2M_ASSET_DIFFUSE) N2M_ASSET_LAUNCH(N2M_ASSET_DIFFUSE, N2M_ASSET_NEAREST);
        else N2M_ASSET_LAUNCH(N2M_ASSET_SPECULAR, N2M_ASSET_NEAREST);
    } else {
        if (mode == N2M_ASSET_FULL) N2M_ASSET_LAUNCH(N2M_ASSET_FULL, N2M_ASSET_LINEAR);
        else if (mode == N2M_ASSET_DIFFUSE) N2M_ASSET_LAUNCH(N2M_ASSET_DIFFUSE, N2M_ASSET_LINEAR);
        else N2M_ASSET_LAUNCH(N2M_ASSET_SPECULAR, N2M_ASSET_LINEAR);
    }
#undef N2M_ASSET_LAUNCH
    N2M_CHECK_LAUNCH();
    return 0;
}
